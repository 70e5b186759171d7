"""Exact-arithmetic tests of the trilinear lookups of OctreeGrid / CodebookOctreeGrid and of their order-free backward
(csrc/spc_interp.hip, csrc/spc_grad.hip).

The inputs of tests/spc_exact_ref.py make every product and every partial sum exactly representable, so every element a kernel
writes must equal the plain float64 reference BIT FOR BIT whatever the merge order, the corner links, the order of the atomics or
the binary point of the fixed-point accumulators: `torch.equal`, no tolerance anywhere in this file.  A bitwise mismatch on exact
inputs is a defect of the kernel (tests/test_spc_exact_host.py rules out the reference and says which paths each sample order
reaches); the assertion message names level, row and channel of the first mismatches.

Every backward test also checks that the scratch behind its 64-byte header is zero afterwards, calls twice and compares, and
hands the kernels buffers with rows behind their end that must never be used.
"""
import pytest
import torch

import spc_exact_ref as R
from gpu_helpers import DEV, _C, _sparse_blas

pytestmark = pytest.mark.gpu

TAIL = 32                       # rows behind the end of coords / grad_out / chain, filled with values that must never be used
_cache = {}


@pytest.fixture(scope="module", autouse=True)
def _release_cases():
    """the cases (inputs and references) are shared by the tests of this file and freed when it finishes"""
    yield
    _cache.clear()


def _tree():
    """the builder's tree on the GPU; its points are those of the package's own octree of the same random cells"""
    if "tree" not in _cache:
        t = R.tree()
        blas, _ = _sparse_blas(5, 3000, R.TREE_SEED)
        assert torch.equal(blas.points.cpu(), torch.from_numpy(t.points))
        valid = int(t.first(5))                                      # (a valid finest cell, for the rows behind the chain)
        _cache["tree"] = (t, blas.points.to(DEV), torch.from_numpy(t.trinkets).to(DEV), valid)
    return _cache["tree"]


def _padded(t, fill):
    """a view of the first rows of a buffer whose TAIL further rows hold `fill`"""
    buf = torch.full((t.shape[0] + TAIL,) + tuple(t.shape[1:]), fill, dtype=t.dtype, device=DEV)
    buf[:t.shape[0]] = t
    return buf[:t.shape[0]]


def _dev(case):
    """the inputs of a case on the GPU, with sentinel rows behind coords (a coordinate inside a cell), grad_out (7) and the chain
    (a valid cell)"""
    t, points, trk, valid = _tree()
    return dict(coords=_padded(case["coords"], 0.015625), grad_out=_padded(case["grad_out"], 7.0),
                chain=_padded(case["chain"], valid), points=points, trinkets=trk)


def _get(key, build, ref=R.reference):
    """(case, reference, device inputs), built once per key"""
    if key not in _cache:
        case = build()
        _cache[key] = (case, ref(case), _dev(case))
    return _cache[key]


def _shapes(case):
    return [(case["tree"].rows(l), case["channels"]) for l in case["levels"]]


def _scratch_is_clean():
    ws = _C()._spc_bwd_workspace(torch.device(DEV), 1, 1)
    assert int(ws[64:].count_nonzero()) == 0, "the backward left its scratch dirty"     # (the 64-byte header is reset by every call)


def _same(got, want, what, levels=None):
    """lists of tensors, bit for bit (compared on the host, with the bit patterns of the magnitudes as well: an equality that
    flushed denormals would not do)"""
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        g, w = g.detach().cpu(), w.detach().cpu()
        assert g.dtype == w.dtype == torch.float32 and g.shape == w.shape, (what, i, g.dtype, g.shape, w.shape)
        if torch.equal(g, w) and torch.equal(g.abs().view(torch.int32), w.abs().view(torch.int32)):
            continue
        bad = torch.nonzero((g != w) | (g.abs().view(torch.int32) != w.abs().view(torch.int32)))
        first = [(tuple(b.tolist()), float(g[tuple(b)]), float(w[tuple(b)])) for b in bad[:6]]
        where = f"level {levels[i]}" if levels is not None else f"tensor {i}"
        raise AssertionError(f"{what}, {where}: {bad.shape[0]} of {g.numel()} elements differ; ((row, channel), got, want): {first}")


def _multi_bwd(case, dev, seeded):
    out = [s.to(DEV) for s in case["seeds"]] if seeded else None
    got = _C().spc_trilinear_multi_backward(dev["coords"], dev["chain"], dev["points"], dev["trinkets"], dev["grad_out"],
                                            _shapes(case), list(case["levels"]), case["sum"], out=out)
    torch.cuda.synchronize()
    return got


def _check_multi_bwd(case, ref, dev, what, seeded=(False, True), scale=1.0):
    """unseeded and onto integer seeds, each twice into fresh outputs; the scratch is clean after every call"""
    for s in seeded:
        want = [(g * scale + (sd.double() if s else 0.0)).float() for g, sd in zip(ref["grads"], case["seeds"])]
        got = _multi_bwd(case, dev, s)
        _scratch_is_clean()
        _same(got, want, f"{what} ({'seeded' if s else 'unseeded'})", case["levels"])
        again = _multi_bwd(case, dev, s)
        _scratch_is_clean()
        _same(again, got, f"{what}: second call", case["levels"])
    return got


def _flags_on(case, n=None):
    """sg_use_flags of spc_grad.hip from the public sizes: touched-row flags when a launch reaches a small part of the table"""
    n = case["N"] if n is None else n
    return n * 8 * len(case["levels"]) < sum(case["tree"].rows(l) for l in case["levels"])


def _levels_split(case, n=None):
    """sg_split_lods: the wide kernel gives every (sample, level) its own lane group while there are few samples"""
    n = case["N"] if n is None else n
    return len(case["levels"]) > 1 and n * min(case["channels"], 64) < 256 * 1024


# ---------------------------------------------------------------------------------------------------- 1. all levels in one launch
@pytest.mark.parametrize("order", ["few", "many", "mixed"])
@pytest.mark.parametrize("mtype", ["sum", "cat"])
def test_backward_of_all_levels_equals_float64_reference(mtype, order):
    """5 channels (the merge kernel): long runs (no wave links corners), ray-like walks (most waves do), and runs of 1 .. 200
    with misses inside, laid end to end"""
    case, ref, dev = _get(("multi", order, 5, mtype), lambda: R.multi_case(order, 5, mtype == "sum"))
    _check_multi_bwd(case, ref, dev, f"{order} {mtype} 5 channels")


@pytest.mark.parametrize("channels", R.MERGE_CHANNELS + R.WIDE_CHANNELS)
def test_backward_at_every_channel_count(channels):
    """each template of the merge kernel (1 .. 8) and the lanes-over-channels kernel at 9, at 12 (four idle threads per block), 16,
    33, 64 and 72 (a second trip of the channel loop), 'sum' and 'cat', on the mixed order"""
    for mtype in ("sum", "cat"):
        case, ref, dev = _get(("multi", "mixed", channels, mtype), lambda: R.multi_case("mixed", channels, mtype == "sum"))
        _check_multi_bwd(case, ref, dev, f"mixed {mtype} {channels} channels")


def test_backward_with_gradients_of_mixed_magnitude():
    case, ref, dev = _get(("mix", 5), lambda: R.multi_case("mixed", 5, True, grad="mix"))
    _check_multi_bwd(case, ref, dev, "mixed magnitudes, 5 channels")
    case, ref, dev = _get(("mix", 16), lambda: R.multi_case("mixed", 16, False, grad="mix"))
    _check_multi_bwd(case, ref, dev, "mixed magnitudes, 16 channels")


# ---------------------------------------------------------------------------------------------------- 2. dispatch switches
@pytest.mark.parametrize("n", R.SMALL_N)
def test_sample_counts_around_wave_and_block(n):
    """the first n samples of the mixed order (a run crosses lane 63 from n = 65 on, and sample 128 from n = 129 on); all these
    launches use touched-row flags and, at 16 channels, one lane group per (sample, level)"""
    for channels in (5, 16):
        base = _get(("multi", "mixed", channels, "sum"), lambda: R.multi_case("mixed", channels, True))[0]
        case, ref, dev = _get(("first", n, channels), lambda: R.truncated(base, n))
        assert _flags_on(case) and _levels_split(case)
        _check_multi_bwd(case, ref, dev, f"n = {n}, {channels} channels")


def test_both_sides_of_the_dispatch_switches():
    """touched-row flags on (n 8 L < rows) and off; levels split (16 n < 256 * 1024) and walked by one lane group"""
    small = _get(("first", 129, 16), lambda: R.truncated(R.multi_case("mixed", 16, True), 129))
    main = _get(("multi", "mixed", 16, "sum"), lambda: R.multi_case("mixed", 16, True))
    big = _get(("big", 16), lambda: R.multi_case("mixed", 16, True, n=R.N_SPLIT_BIG))
    assert _flags_on(small[0]) and not _flags_on(main[0]) and not _flags_on(big[0])
    assert _levels_split(small[0]) and _levels_split(main[0]) and not _levels_split(big[0])
    assert _levels_split(big[0], R.N_SPLIT_BIG - 200) and abs(R.N_SPLIT_BIG * 16 - 256 * 1024) < 4096     # (just past the switch)
    five = _get(("multi", "mixed", 5, "sum"), lambda: R.multi_case("mixed", 5, True))
    assert not _flags_on(five[0]) and _flags_on(five[0], 129)
    for name, (case, ref, dev) in (("129 samples", small), ("3000 samples", main), ("16500 samples", big)):
        _check_multi_bwd(case, ref, dev, f"16 channels, {name}", seeded=(True,))


@pytest.mark.parametrize("levels", [(5,), (4, 5), (3, 4, 5)])
def test_backward_with_fewer_active_levels(levels):
    for channels in (5, 16):
        case, ref, dev = _get(("levels", levels, channels), lambda: R.multi_case("mixed", channels, False, levels=levels))
        _check_multi_bwd(case, ref, dev, f"levels {levels}, {channels} channels", seeded=(True,))


# ---------------------------------------------------------------------------------------------------- 3. single-level leaf call
@pytest.mark.parametrize("channels", [5, 16])
@pytest.mark.parametrize("idx", [torch.int32, torch.int64], ids=["i32", "i64"])
@pytest.mark.parametrize("S", [1, 4, 16])
def test_leaf_call_with_samples_per_voxel(S, idx, channels):
    """spc_trilinear_forward / _backward on coords [V, S, 3] in voxels pidx [V] of the finest level, offsets k / 8, every 17th
    pidx -1; fp32 tables, and fp16 tables with the reference's half rounding (integer features, weights of 9 fractional bits)"""
    case, ref, dev = _get(("leaf", S, channels), lambda: R.leaf_case(5, S, channels))
    assert ref["half_ok"]
    C, level = _C(), case["levels"][0]
    V = case["N"] // S
    coords = dev["coords"].view(V, S, 3)
    pidx = _padded(case["chain"][::S, 0].to(idx).contiguous(), _tree()[3])
    assert int((pidx < 0).sum()) > 0
    feats = case["feats"][0].to(DEV)
    want = [ref["out"].float().view(V, S, channels)]
    _same([C.spc_trilinear_forward(coords, pidx, dev["points"], dev["trinkets"], feats, level, False)], want, "leaf forward")
    _same([C.spc_trilinear_forward(coords, pidx, dev["points"], dev["trinkets"], feats.half(), level, True)], want, "leaf forward fp16")
    g = dev["grad_out"].view(V, S, channels)
    for seeded in (False, True):
        wantg = [(ref["grads"][0] + (case["seeds"][0].double() if seeded else 0.0)).float()]
        outs = []
        for _ in range(2):
            out = case["seeds"][0].to(DEV) if seeded else None
            outs.append(C.spc_trilinear_backward(coords, pidx, dev["points"], dev["trinkets"], g, _shapes(case)[0], level, out=out))
            torch.cuda.synchronize()
            _scratch_is_clean()
        _same(outs[:1], wantg, f"leaf backward S = {S} ({'seeded' if seeded else 'unseeded'})", case["levels"])
        _same(outs[1:], outs[:1], "leaf backward: second call", case["levels"])


# ---------------------------------------------------------------------------------------------------- 4. forward
@pytest.mark.parametrize("channels,n", [(5, R.N_MAIN), (5, 4500), (16, R.N_MAIN), (72, R.N_MAIN)])
@pytest.mark.parametrize("mtype", ["sum", "cat"])
def test_forward_of_all_levels_equals_float64_reference(mtype, channels, n):
    """spc_trilinear_multi_forward: the lanes-over-channels kernel and, from 4096 samples on, the thread-per-sample one (<= 8
    channels); four levels in fp32.  fp16 tables with half rounding on the two finest levels only: a per-level result of the two
    coarser ones has 2^-9 / 2^-12 steps and is no fp16 value (the builder's half_ok says so)"""
    C = _C()
    for levels in (R.LEVELS4, (4, 5)):
        case, ref, dev = _get(("fwd", levels, channels, mtype, n), lambda: R.multi_case("mixed", channels, mtype == "sum", levels, n=n))
        feats = [f.to(DEV) for f in case["feats"]]
        out = C.spc_trilinear_multi_forward(dev["coords"], dev["chain"], dev["points"], dev["trinkets"], feats, list(levels), False,
                                            case["sum"])
        _same([out], [ref["out"].float()], f"forward {mtype} {channels} channels, levels {levels}")
        assert ref["half_ok"] == (len(levels) == 2)
        if ref["half_ok"]:
            out = C.spc_trilinear_multi_forward(dev["coords"], dev["chain"], dev["points"], dev["trinkets"], [f.half() for f in feats],
                                                list(levels), True, case["sum"])
            _same([out], [ref["out"].float()], f"forward fp16 {mtype} {channels} channels, levels {levels}")


# ---------------------------------------------------------------------------------------------------- 5. loss scale
@pytest.mark.parametrize("exp", R.LOSS_SCALES)
@pytest.mark.parametrize("channels", [5, 16])
def test_backward_is_exact_under_any_loss_scale(channels, exp):
    """the gradient times 2^16, 2^24, 2^-30 and 2^-130 (a denormal maximum: the `e < 1` clamp of the fixed-point scale; every
    product is a multiple of 2^-142): the result is the reference times the same power of two"""
    base = _get(("multi", "mixed", channels, "sum"), lambda: R.multi_case("mixed", channels, True))
    case, ref, dev = _get(("scale", channels, exp), lambda: R.multi_case("mixed", channels, True, scale_exp=exp))
    assert torch.equal(case["grad_out"].double(), base[0]["grad_out"].double() * 2.0 ** exp)
    assert all(torch.equal(a, b * 2.0 ** exp) for a, b in zip(ref["grads"], base[1]["grads"]))
    _check_multi_bwd(case, base[1], dev, f"gradient x 2^{exp}, {channels} channels", seeded=(False,), scale=2.0 ** exp)


# ---------------------------------------------------------------------------------------------------- 6. nearly overflowing
@pytest.mark.parametrize("channels", [5, 16])
def test_finite_gradients_near_overflow_take_the_float_path_exactly(channels):
    """|g| in {0, 2^121} with offset 0 present: M >= 2^121, the path of inf / NaN, with finite values - which must still be
    right (at most 32 contributions per row, no sum reaches 2^127; exactness makes the order of the float atomics irrelevant)"""
    case, ref, dev = _get(("huge", channels), lambda: R.huge_case(channels))
    assert float(case["grad_out"].abs().max()) == 2.0 ** R.HUGE_EXP and max(float(g.abs().max()) for g in ref["grads"]) >= 2.0 ** R.HUGE_EXP
    got = _check_multi_bwd(case, ref, dev, f"2^121, {channels} channels", seeded=(False,))
    assert all(bool(torch.isfinite(g).all()) for g in got)


# ---------------------------------------------------------------------------------------------------- 7. degenerate launches
def test_zero_gradient_leaves_a_seeded_out_unchanged():
    for channels in (5, 16):
        case, ref, dev = _get(("multi", "mixed", channels, "sum"), lambda: R.multi_case("mixed", channels, True))
        dev = dict(dev, grad_out=_padded(torch.zeros_like(case["grad_out"]), 7.0))
        _same(_multi_bwd(case, dev, True), case["seeds"], f"zero gradient, {channels} channels", case["levels"])
        _scratch_is_clean()


def test_no_samples():
    for channels in (5, 16):
        case = R.truncated(R.multi_case("mixed", channels, True), 0)
        _same(_multi_bwd(case, _dev(case), True), case["seeds"], f"n = 0, {channels} channels", case["levels"])
        _scratch_is_clean()


def test_all_samples_outside_every_cell():
    for channels in (5, 16):
        case = R.make_case(R.tree(), -torch.ones(700, 3).long().numpy(), R.LEVELS4, channels, True, seed=5)
        assert bool((case["chain"] < 0).all())
        _same(_multi_bwd(case, _dev(case), True), case["seeds"], f"all outside, {channels} channels", case["levels"])
        _scratch_is_clean()


def test_rows_whose_contributions_cancel_keep_their_seed():
    for channels in (5, 16):
        case, ref, dev = _get(("cancel", channels), lambda: R.cancel_case(channels))
        gone = R.cancelled_rows(ref)
        assert all(int(m.sum()) > 0 for m in gone) and all(float(g.abs().max()) > 0 for g in ref["grads"])
        got = _check_multi_bwd(case, ref, dev, f"cancelling rows, {channels} channels", seeded=(True,))
        for g, s, m in zip(got, case["seeds"], gone):
            assert torch.equal(g.cpu()[m], s[m])


# ---------------------------------------------------------------------------------------------------- 8. codebook
def _unaligned(t):
    """a copy of t whose storage starts 4 bytes behind a 16-byte boundary (no 16-byte loads of its rows)"""
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=DEV)
    out = buf[1:].view(t.shape)
    out.copy_(t)
    assert out.data_ptr() % 16 == 4
    return out


# (dictionary size, feature dim, logits 16-byte aligned): K <= 16, a multiple of four, and aligned rows reach the register
# template codebook_grad_finalize_kernel<16>; unaligned rows the generic <0>
CODEBOOKS = {"K16_F5_registers": (16, 5, True), "K8_F3_generic": (8, 3, False)}


def _codebook_ref(cb):
    return lambda case: R.codebook_reference(case, cb)


def _codebook(mode, name, mtype):
    K, F, aligned = CODEBOOKS[name]
    key = ("codebook", mode, name, mtype)
    if key not in _cache:
        case, cb = R.codebook_case(mode, K, F, mtype == "sum")
        place = (lambda t: t.to(DEV)) if aligned else (lambda t: _unaligned(t.to(DEV)))
        _cache[key] = (case, cb, R.codebook_reference(case, cb), _dev(case), [place(t) for t in cb["logits"]], [t.to(DEV) for t in cb["dicts"]])
    return _cache[key]


@pytest.mark.parametrize("name", list(CODEBOOKS))
@pytest.mark.parametrize("mtype", ["sum", "cat"])
@pytest.mark.parametrize("mode", ["onehot", "uniform"])
def test_codebook_backward_of_all_levels_equals_float64_reference(mode, mtype, name):
    """one-hot logits: d logits exactly 0, d dictionary[key] = sum G.  Uniform logits: p = 1 / K, d logits = (D_k . G - mean) / K and
    the whole G goes to key 0 (first index on ties).  Onto integer seeds and onto zeros, twice each."""
    case, cb, ref, dev, logits, dicts = _codebook(mode, name, mtype)
    assert all((t.data_ptr() % 16 == 0) == CODEBOOKS[name][2] for t in logits)
    if mode == "uniform":
        assert max(float(g.abs().max()) for g in ref["grad_logits"]) > 0
    for seeded in (False, True):
        want_l = [(g + (s.double() if seeded else 0.0)).float() for g, s in zip(ref["grad_logits"], cb["seeds_logits"])]
        want_d = [(g + (s.double() if seeded else 0.0)).float() for g, s in zip(ref["grad_dicts"], cb["seeds_dict"])]
        outs = []
        for _ in range(2):
            out = ([s.to(DEV) for s in cb["seeds_logits"]], [s.to(DEV) for s in cb["seeds_dict"]]) if seeded else None
            outs.append(_C().codebook_trilinear_multi_backward(dev["coords"], dev["chain"], dev["points"], dev["trinkets"], logits, dicts,
                                                               dev["grad_out"], list(case["levels"]), case["sum"], out=out))
            torch.cuda.synchronize()
            _scratch_is_clean()
        tag = f"codebook {mode} {mtype} {name} ({'seeded' if seeded else 'unseeded'})"
        _same(outs[0][0], want_l, tag + " grad_logits", case["levels"])
        _same(outs[0][1], want_d, tag + " grad_dictionary", case["levels"])
        _same(outs[1][0], outs[0][0], tag + " grad_logits of a second call", case["levels"])
        _same(outs[1][1], outs[0][1], tag + " grad_dictionary of a second call", case["levels"])


@pytest.mark.parametrize("K,F,aligned", [(16, 5, True), (8, 3, False), (8, 3, True)], ids=["K16_F5_registers", "K8_F3_generic", "K8_F3_registers"])
@pytest.mark.parametrize("level,S,V", [(5, 4, 600), (3, 4, 800)], ids=["fused_lookup", "decoded_rows"])
@pytest.mark.parametrize("mode", ["onehot", "uniform"])
def test_codebook_leaf_call_equals_float64_reference(mode, level, S, V, K, F, aligned):
    """codebook_trilinear_backward on coords [V, S, 3] of one level, and the forward - training and evaluation, the fused lookup
    (few samples per table row) and the decoded-rows route (V S >= 4 rows), and codebook_decode_rows itself"""
    key = ("cbleaf", mode, level, K, F)
    if key not in _cache:
        case, cb = R.codebook_leaf_case(mode, K, F, level, S, V)
        _cache[key] = (case, cb, R.codebook_reference(case, cb), _dev(case))
    case, cb, ref, dev = _cache[key]
    C = _C()
    rows = case["tree"].rows(level)
    assert (V * S >= 4 * rows) == (level == 3)
    coords, g = dev["coords"].view(V, S, 3), dev["grad_out"].view(V, S, F)
    pidx = _padded(case["chain"][::S, 0].contiguous(), _tree()[3])
    logits = cb["logits"][0].to(DEV) if aligned else _unaligned(cb["logits"][0].to(DEV))
    D = cb["dicts"][0].to(DEV)
    want = [ref["out"].float().view(V, S, F)]
    for training in (True, False):
        _same([C.codebook_decode_rows(logits, D, training)], [R.codebook_tables(cb)[0]], f"decode_rows {mode} training={training}")
        _same([C.codebook_trilinear_forward(coords, pidx, dev["points"], dev["trinkets"], logits, D, level, training)], want,
              f"codebook forward {mode} training={training}")
    for seeded in (False, True):
        outs = []
        for _ in range(2):
            out = (cb["seeds_logits"][0].to(DEV), cb["seeds_dict"][0].to(DEV)) if seeded else None
            outs.append(C.codebook_trilinear_backward(coords, pidx, dev["points"], dev["trinkets"], logits, D, g, level, out=out))
            torch.cuda.synchronize()
            _scratch_is_clean()
        tag = f"codebook leaf {mode} K={K} ({'seeded' if seeded else 'unseeded'})"
        _same([outs[0][0]], [(ref["grad_logits"][0] + (cb["seeds_logits"][0].double() if seeded else 0.0)).float()], tag + " grad_logits", [level])
        _same([outs[0][1]], [(ref["grad_dicts"][0] + (cb["seeds_dict"][0].double() if seeded else 0.0)).float()], tag + " grad_dictionary", [level])
        _same(list(outs[1]), list(outs[0]), tag + " second call")


# ---------------------------------------------------------------------------------------------------- 9. cross-path
@pytest.mark.parametrize("mtype", ["sum", "cat"])
def test_sample_order_does_not_change_a_bit(mtype):
    """the ray-like order (most waves link corners across tails) and the same samples regrouped by cell (no wave does) give the
    same gradients - and both equal the reference"""
    walk = _get(("multi", "many", 5, mtype), lambda: R.multi_case("many", 5, mtype == "sum"))
    perm = R.regroup(R.tree(), 5, R.cells_of("many"))
    long_runs = _get(("regrouped", mtype), lambda: R.permuted(walk[0], perm))
    a = _check_multi_bwd(*walk, f"walk {mtype}", seeded=(True,))
    b = _check_multi_bwd(*long_runs, f"walk regrouped {mtype}", seeded=(True,))
    _same(a, b, "walk against its regrouped order", walk[0]["levels"])
