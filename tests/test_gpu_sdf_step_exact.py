"""GPU: the two fused octree SDF training steps (wisp_sdf_train_step, wisp_sdf_tex_train_step, csrc/spc_grad.hip) against the float64
restatement of tests/sdf_step_exact_ref.py, element for element.
Family A: exactly representable inputs (the reference file proves per case that no product and no partial sum rounds, in any order
of addition): loss and every gradient, ADDED to pre-filled buffers, must equal float64 BIT FOR BIT (torch.equal only) - over the level
lists that give 16, 8, 5, 4, 3, 2 and 1 samples per pass, batch sizes with tail passes, idle lane groups and a second grid-stride
pass, hidden widths 1 .. 256, half_round, both input layouts and the colour modes of the textured step, samples on the relu edge,
batches that miss every cell, a second call on the same buffers, the forward value, the one-output / four-output relation, and what
the scratch may hold behind its declared size.
Family B: the same inputs at batch sizes that are no power of two - only the sums of the gradients round - with every element inside
a bound derived from its own terms (sdf_step_exact_ref.derived_bounds; nothing in it is measured).  One target of +inf per step.
Every measured ratio to its bound is appended to profiles/sdf_step_exact_test_margins.jsonl when WISP_SDF_STEP_EXACT_MARGINS names
a file."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

import sdf_step_exact_ref as X

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GRADS = ("w1", "b1", "w2", "b2")


def record(name, **values):
    path = os.environ.get("WISP_SDF_STEP_EXACT_MARGINS")
    if path:
        with open(path, "a") as f:
            f.write(json.dumps(dict(name=name, **{k: (float(v) if not isinstance(v, (int, str)) else v) for k, v in values.items()})) + "\n")


_dev_trees = {}


def dev_tree(case):
    name = case["tree_name"]
    if name not in _dev_trees:
        tr = case["tree"]
        _dev_trees[name] = dict(octree=torch.from_numpy(np.asarray(tr.octree).astype(np.uint8)).to(DEV),
                                exsum=torch.from_numpy(np.asarray(tr.exsum).astype(np.int32)).to(DEV),
                                points=torch.from_numpy(np.asarray(tr.points).astype(np.int16)).to(DEV),
                                trinkets=torch.from_numpy(np.asarray(tr.trinkets).astype(np.int32)).to(DEV))
    return _dev_trees[name]


def shapes(case):
    """the decoder buffers' shapes as the entry points take them: the one-output step has w2 [H] and b2 [1]"""
    H = case["w1"].shape[0]
    return dict(w1=tuple(case["w1"].shape), b1=(H,), w2=(4, H) if case["tex"] else (H,), b2=(4,) if case["tex"] else (1,))


def prefill(case, zero=False):
    """gradient buffers holding non-zero multiples of 1/2 up to X.PREFILL_MAX (host copies): the step must ADD to them"""
    def fill(shape, k):
        n = int(np.prod(shape))
        v = (((torch.arange(n) + k) % 7).float() - 3.0) / 2.0
        v[v == 0] = X.PREFILL_MAX
        return (torch.zeros(n) if zero else v).reshape(shape)
    out = {k: fill(s, i) for i, (k, s) in enumerate(shapes(case).items())}
    out["tables"] = [fill(tuple(t.shape), 4 + li) for li, t in enumerate(case["tables"])]
    return out


def _inputs(case, gts=None, rgb=None):
    sh = shapes(case)
    t = dev_tree(case)
    return dict(t, coords=case["coords"].to(DEV).contiguous(), gts=(case["gts"] if gts is None else gts).float().reshape(-1, 1).to(DEV),
                rgb=(case["rgb_gts"] if rgb is None else rgb).float().to(DEV).contiguous(),
                feats=[f.to(DEV).contiguous() for f in case["tables"]], levels=[int(l) for l in case["levels"]],
                **{k: case[k].reshape(sh[k]).to(DEV).contiguous() for k in GRADS})


def run_step(case, before, gts=None, rgb=None, calls=1):
    """`calls` launches on buffers holding `before` -> dict of host tensors: the loss and the buffers afterwards"""
    import wisp._C as C
    i = _inputs(case, gts, rgb)
    bufs = {k: before[k].to(DEV).contiguous() for k in GRADS}
    tabs = [t.to(DEV).contiguous() for t in before["tables"]]
    for _ in range(calls):
        if case["tex"]:
            loss = C.sdf_tex_train_step(i["coords"], i["gts"], i["rgb"], i["octree"], i["exsum"], i["points"], i["trinkets"], i["feats"],
                                        i["levels"], case["half_round"], case["pos_input"], i["w1"], i["b1"], i["w2"], i["b2"], tabs,
                                        bufs["w1"], bufs["b1"], bufs["w2"], bufs["b2"])
        else:
            loss = C.sdf_train_step(i["coords"], i["gts"], i["octree"], i["exsum"], i["points"], i["trinkets"], i["feats"], i["levels"],
                                    case["half_round"], i["w1"], i["b1"], i["w2"], i["b2"], tabs, bufs["w1"], bufs["b1"], bufs["w2"],
                                    bufs["b2"])
    assert loss.shape == ((3,) if case["tex"] else (1,)) and loss.dtype == torch.float32
    return dict(loss=loss.cpu(), tables=[t.cpu() for t in tabs], **{k: v.cpu() for k, v in bufs.items()})


def assert_bits(case, got, before, want=None, times=1):
    want = case["want"] if want is None else want
    assert torch.equal(got["loss"].double(), want["loss"]), ("loss", got["loss"].tolist(), want["loss"].tolist())
    for k in GRADS:
        exp = before[k].double() + times * want[k].reshape(before[k].shape)
        assert torch.equal(exp.float().double(), exp), f"inputs are not exact: {k}"
        bad = got[k].double() != exp
        assert not bool(bad.any()), (k, int(bad.sum()), bad.nonzero()[:4].tolist())
    for li, (g, b, w) in enumerate(zip(got["tables"], before["tables"], want["tables"])):
        exp = b.double() + times * w
        assert torch.equal(exp.float().double(), exp), f"inputs are not exact: table {li}"
        bad = g.double() != exp
        assert not bool(bad.any()), ("table", li, int(bad.sum()), bad.nonzero()[:4].tolist())


def check_exact(case):
    before = prefill(case)
    got = run_step(case, before)
    assert_bits(case, got, before)
    rep = case["report"]
    record("exact", tex=int(case["tex"]), levels=str(case["levels"]), n=case["n"], hidden=case["hidden"], b=case["b"], align=case["align"],
           half_round=int(case["half_round"]), pos_input=case["pos_input"], bits_used=max(rep["spans"].values()), relu_edge=rep["edge"],
           table_entries_moved=sum(int((w != 0).sum()) for w in case["want"]["tables"]))
    return got, before


LISTS = list(range(len(X.LEVEL_LISTS)))


# ------------------------------------------------------------------------------------------------ family A: level lists x n
@pytest.mark.parametrize("n", X.NS)
@pytest.mark.parametrize("li", LISTS, ids=[f"{t}{len(l)}from{l[0]}" for t, l in X.LEVEL_LISTS])
@pytest.mark.parametrize("tex", [0, 1])
def test_step_equals_float64_bit_for_bit(tex, li, n):
    """every level list (16, 8, 5, 4, 3, 2, 2 and 1 samples per pass, lists that start above level 1, lists with gaps) at n = 1, 2, 16,
    64, 512: samples outside the cube, in empty cells whose ancestors exist and on the relu edge are among the inputs; the textured
    step alternates its input layout"""
    tree, levels = X.LEVEL_LISTS[li]
    kw = dict(tex=True, pos_input=(li + n) % 2) if tex else {}
    check_exact(X.exact_case(tree, levels, n, 24 if tex else 16, **kw))


@pytest.mark.parametrize("which", [0, 1])
@pytest.mark.parametrize("tex", [0, 1])
def test_second_grid_stride_pass(tex, which):
    """n = 4096 at 6 levels: 2 samples per pass, 1024 workgroups, every one makes two passes; n = 8192 at 3 levels: 5 per pass, some
    workgroups make two passes and some one"""
    tree, levels, n = X.BIG[which]
    shape = X.launch_shape(len(levels), n)
    assert shape["grid"] == X.GRID_CAP and (shape["second_pass_all"] if which == 0 else shape["second_pass_some"])
    check_exact(X.exact_case(tree, levels, n, 16, tex=bool(tex)))


# ------------------------------------------------------------------------------------------------ family A: the decoder
@pytest.mark.parametrize("hidden", [1, 16, 17, 24, 256])
@pytest.mark.parametrize("tex,pos", [(0, 1), (1, 1), (1, 0)])
def test_hidden_widths(tex, pos, hidden):
    """1 unit, a multiple of 16, two that are none, and ST_MAX_HIDDEN = 256 (dynamic LDS above 64 KB)"""
    check_exact(X.exact_case("small", (3, 4, 5), 64, hidden, tex=bool(tex), pos_input=pos))


@pytest.mark.parametrize("tex", [0, 1])
def test_every_unit_of_128_is_live_over_the_pattern_sweep(tex):
    """the non-zero output weights rotate over the 128 units: every element of dW1, db1, dw2 / dW2 and db2 is non-zero in one pattern
    at least (asserted on the float64 side by tests/test_sdf_step_exact_host.py) and equal in all"""
    for pattern in range(X.n_patterns(128, bool(tex))):
        check_exact(X.exact_case("small", (3, 4, 5), 64, 128, tex=bool(tex), pattern=pattern))


@pytest.mark.parametrize("n", [16, 512])
@pytest.mark.parametrize("levels", [(5,), (4, 5), (3, 4, 5), (0, 1, 2, 3, 4, 5)])
@pytest.mark.parametrize("tex,pos", [(0, 1), (1, 1), (1, 0)])
def test_half_round(tex, pos, levels, n):
    """a third of the non-zero table entries is an integer + 2^-13 that only the fp16 rounding of the table turns back into the
    integer, and every level's blend is an fp16 value (asserted): the rounding of the inputs is seen, the rounding of the blends
    must change nothing"""
    check_exact(X.exact_case("small", levels, n, 24, tex=bool(tex), pos_input=pos, half_round=True))


@pytest.mark.parametrize("modes", [("half",) * 3, ("low",) * 3, ("high",) * 3, ("low", "half", "high")], ids="-".join)
@pytest.mark.parametrize("pos", [0, 1])
def test_colour_modes(pos, modes):
    case = X.exact_case("small", (2, 3, 4, 5), 64, 24, tex=True, pos_input=pos, modes=modes)
    got, before = check_exact(case)
    for o, m in enumerate(modes):                      # a saturated colour has no gradient: its rows keep the pre-filled bits
        if m != "half":
            assert torch.equal(got["w2"][o], before["w2"][o]) and torch.equal(got["b2"][o], before["b2"][o])
        else:
            assert not torch.equal(got["w2"][o], before["w2"][o])
    assert float(got["loss"][2]) > 0


# ------------------------------------------------------------------------------------------------ family A: edges of the batch
@pytest.mark.parametrize("tex", [0, 1])
def test_a_batch_that_misses_every_cell(tex):
    """half of the samples outside the cube, half in cells that are empty at every listed level: the tables keep their bits, the
    decoder's gradients are those of the position alone"""
    case = X.exact_case("deep", (8, 9, 10), 64, 24, tex=bool(tex), all_miss=True)
    assert bool((case["chain"] < 0).all()) and bool((case["coords"].abs() <= 1).all(1).any()) and bool((case["coords"].abs() > 1).any())
    got, before = check_exact(case)
    for g, b in zip(got["tables"], before["tables"]):
        assert torch.equal(g, b)
    assert torch.equal(got["w1"][:, 3:], before["w1"][:, 3:]) and not torch.equal(got["w1"][:, :3], before["w1"][:, :3])


@pytest.mark.parametrize("tex", [0, 1])
def test_a_second_call_adds_the_same_amounts_again(tex):
    case = X.exact_case("small", (2, 3, 4, 5), 64, 24, tex=bool(tex))
    before = prefill(case)
    got = run_step(case, before, calls=2)
    assert_bits(case, got, before, times=2)


@pytest.mark.parametrize("tex", [0, 1])
@pytest.mark.parametrize("li", [2, 5, 7, 8])
def test_forward_is_the_querys_value_bit_for_bit(li, tex):
    """one exact sample: d b2 = g = 2 (pred - gt), so pred = gt + g / 2 exactly - the value wisp_sdf_query returns"""
    import wisp._C as C
    tree, levels = X.LEVEL_LISTS[li]
    case = X.exact_case(tree, levels, 1, 24, tex=bool(tex))
    got = run_step(case, prefill(case, zero=True))
    pred = case["gts"].double().reshape(-1) + got["b2"].double()[-1:] / 2.0
    i = _inputs(case)
    fld = dict(dev_tree(case), feats=i["feats"], levels=i["levels"], half_round=False, w1=i["w1"], b1=i["b1"], w2=i["w2"], b2=i["b2"])
    query = C.sdf_query(i["coords"], fld).cpu().double()
    assert torch.equal(pred, query[:, -1]) and torch.equal(pred, case["want"]["pred"])
    assert float(got["b2"][-1]) != 0.0


@pytest.mark.parametrize("n", [64, 512])
def test_inert_colour_rows_give_the_one_output_steps_bits(n):
    """W2[0:3] = 0, b2[0:3] = 0, colour target 1/2: the tables, dW1 and db1 of the four-output step are the one-output step's bits
    (test_gpu_sdf_tex_step.py holds that relation on generic inputs) - and here both sides are float64's as well"""
    tex = X.exact_case("small", (2, 3, 4, 5), n, 24, tex=True, inert_colour=True)
    one = dict(tex, tex=False, w2=tex["w2"][3:4].clone(), b2=tex["b2"][3:4].clone())
    one["want"] = X.step_reference(one)
    X.check_exact_step(one)
    b_tex, b_one = prefill(tex), prefill(one)
    b_one["w1"], b_one["b1"], b_one["tables"] = b_tex["w1"], b_tex["b1"], b_tex["tables"]
    g_tex, g_one = run_step(tex, b_tex), run_step(one, b_one)
    assert_bits(tex, g_tex, b_tex)
    assert_bits(one, g_one, b_one)
    assert torch.equal(g_tex["w1"], g_one["w1"]) and torch.equal(g_tex["b1"], g_one["b1"])
    assert all(torch.equal(a, b) for a, b in zip(g_tex["tables"], g_one["tables"]))
    assert float(g_tex["loss"][2]) == 0.0 and float(g_tex["loss"][0]) == float(g_one["loss"][0])
    assert torch.equal(g_tex["w2"][:3], b_tex["w2"][:3]) and torch.equal(g_tex["b2"][:3], b_tex["b2"][:3])


# ------------------------------------------------------------------------------------------------ scratch bounds
PAD = 4096
SENTINEL = 0xA5


@pytest.mark.parametrize("tex,li,n,hidden", [(0, 2, 37, 17), (1, 5, 64, 24), (0, 7, 16, 16)])
def test_nothing_is_written_behind_the_declared_scratch_size(tex, li, n, hidden):
    """the C entry point with a scratch of exactly wisp_sdf_train_scratch_bytes / wisp_sdf_tex_train_scratch_bytes inside a larger
    allocation filled with a sentinel: the bytes before and behind it are unchanged, the results those of the cached-scratch call"""
    import wisp._C as C
    tree, levels = X.LEVEL_LISTS[li]
    big = X.exact_case(tree, levels, 64, hidden, tex=bool(tex))
    case = big if n == 64 else X.inexact_case(big, n)
    before = prefill(case)
    cached = run_step(case, before)
    i = _inputs(case)
    L, H = len(levels), hidden
    need = int(C.lib.wisp_sdf_tex_train_scratch_bytes(n, L, X.C, H, case["pos_input"]) if tex else C.lib.wisp_sdf_train_scratch_bytes(n, L, X.C, H))
    assert need > 0
    arena = torch.full((need + 2 * PAD,), SENTINEL, dtype=torch.uint8, device=DEV)
    scratch = ctypes.c_void_p(arena.data_ptr() + PAD)
    bufs = {k: before[k].to(DEV).contiguous() for k in GRADS}
    tabs = [t.to(DEV).contiguous() for t in before["tables"]]
    rarr, rptr = C._host_i64([f.shape[0] for f in i["feats"]])
    ws = C._spc_bwd_workspace(torch.device(DEV), int(rarr.sum()), X.C)
    farr, fptr = C._ptr_array(i["feats"])
    garr, gptr = C._ptr_array(tabs)
    larr, lptr = C._host_i32(i["levels"])
    loss = torch.empty(3 if tex else 1, dtype=torch.float32, device=DEV)
    p = C._p
    head = [p(i["coords"]), p(i["gts"])] + ([p(i["rgb"])] if tex else []) + [n, p(i["octree"]), p(i["exsum"]), p(i["points"]), p(i["trinkets"]),
                                                                              fptr, lptr, rptr, L, X.C, int(case["half_round"])]
    tail = [p(i["w1"]), p(i["b1"]), p(i["w2"]), p(i["b2"]), H, gptr, p(bufs["w1"]), p(bufs["b1"]), p(bufs["w2"]), p(bufs["b2"]), p(loss),
            scratch, need, p(ws), ws.numel(), C._stream()]
    f = C._cdll.wisp_sdf_tex_train_step if tex else C._cdll.wisp_sdf_train_step
    rc = f(*(head + ([case["pos_input"]] if tex else []) + tail))
    torch.cuda.synchronize()
    assert rc == 0, C.lib.wisp_last_error()
    host = arena.cpu()
    assert bool((host[:PAD] == SENTINEL).all()) and bool((host[PAD + need:] == SENTINEL).all())
    assert not bool((host[PAD:PAD + need] == SENTINEL).all())
    assert torch.equal(loss.cpu(), cached["loss"])
    for k in GRADS:
        assert torch.equal(bufs[k].cpu(), cached[k]), k
    assert all(torch.equal(a.cpu(), b) for a, b in zip(tabs, cached["tables"]))


# ------------------------------------------------------------------------------------------------ family B: n no power of two
def check_bounded(case, tag):
    before = prefill(case)
    got = run_step(case, before)
    bounds = X.derived_bounds(case, before)
    want = case["want"]
    worst = {}
    pairs = [("loss", got["loss"].double(), want["loss"], bounds["loss"])]
    pairs += [(k, got[k].double(), before[k].double() + want[k].reshape(before[k].shape), bounds[k].reshape(before[k].shape)) for k in GRADS]
    pairs += [(f"table{li}", g.double(), b.double() + w, bd) for li, (g, b, w, bd) in enumerate(zip(got["tables"], before["tables"], want["tables"], bounds["tables"]))]
    failures = []
    for name, g, w, bd in pairs:
        err = (g - w).abs()
        ratio = torch.where(bd > 0, err / bd.clamp(min=1e-300), torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))
        worst[name] = float(ratio.max())
        print(f"{tag} {name}: worst error / bound {worst[name]:.3f}, largest error {float(err.max()):.3e}")
        if not bool((err <= bd).all()):
            failures.append((name, worst[name], int((err > bd).sum())))
    record("bounded", case=tag, **worst)
    assert not failures, failures
    assert any(v > 0 for v in worst.values()) or case["n"] < 4          # (something does round: the bound is not vacuous)


@pytest.mark.parametrize("n", X.INEXACT_NS)
@pytest.mark.parametrize("tex,pos", [(0, 1), (1, 1), (1, 0)])
def test_sums_stay_within_the_derived_bound_at_other_batch_sizes(tex, pos, n):
    """n = 3, 37, 511, 513 over three levels (5 samples per pass: tail passes and an idle lane group): fl(1 / n) is no power of two, g
    is rounded once and reproduced, the sums of the gradients round - every element within (k + 2) 2^-24 A of float64, k its number
    of non-zero terms and A their absolute sum plus the pre-filled value; table elements add the propagated error of d features and
    one fixed-point quantum per contribution"""
    size = 64 if n < 64 else 512 if n < 512 else 1024
    case = X.inexact_case(X.exact_case("small", (3, 4, 5), size, 24, tex=bool(tex), pos_input=pos), n)
    check_bounded(case, f"tex{tex} pos{pos} n{n}")


@pytest.mark.parametrize("tex", [0, 1])
def test_sums_stay_within_the_derived_bound_at_2049_over_six_levels(tex):
    """2 samples per pass, 1024 workgroups, one of them makes a second pass - with a single sample in it"""
    tree, levels, n = X.INEXACT_BIG
    assert X.launch_shape(len(levels), n)["max_passes"] == 2
    case = X.inexact_case(X.exact_case(tree, levels, 4096, 16, tex=bool(tex)), n)
    check_bounded(case, f"tex{tex} six levels n{n}")


# ------------------------------------------------------------------------------------------------ a non-finite target
@pytest.mark.parametrize("tex", [0, 1])
def test_one_infinite_target(tex):
    """one target of +inf: every element the float64 reference keeps finite - the table rows that sample does not touch, the hidden
    units that are off for it (relu's backward selects: it passes 0 on, not 0 * inf), the colour sums - is bit-equal, every element
    the reference makes non-finite is non-finite (inf against NaN is not compared)"""
    case = X.exact_case("small", (3, 4, 5), 16, 24, tex=bool(tex))
    gts = case["gts"].clone()
    gts[3] = float("inf")
    want = X.step_reference(case, gts=gts)
    before = prefill(case)
    got = run_step(case, before, gts=gts)
    pairs = [("loss", got["loss"].double(), want["loss"])]
    pairs += [(k, got[k].double(), before[k].double() + want[k].reshape(before[k].shape)) for k in GRADS]
    pairs += [(f"table{li}", g.double(), b.double() + w) for li, (g, b, w) in enumerate(zip(got["tables"], before["tables"], want["tables"]))]
    finite_seen = 0
    for name, g, w in pairs:
        fin = torch.isfinite(w)
        assert not bool(torch.isfinite(g[~fin]).any()), (name, "finite where float64 is not", int(torch.isfinite(g[~fin]).sum()))
        bad = g[fin] != w[fin]
        assert not bool(bad.any()), (name, "differs where float64 is finite", int(bad.sum()), g[fin][bad][:4].tolist(), w[fin][bad][:4].tolist())
        if name != "loss":
            finite_seen += int(fin.sum()) if not bool(fin.all()) else 0
    assert not bool(torch.isfinite(want["loss"][0])) and finite_seen > 0
    p = X.decoder_parts(case, gts=gts)
    off = (p["a"][3] <= 0)
    assert bool(off.any()) and bool(torch.isfinite(want["b1"][off]).all()) and not bool(torch.isfinite(want["b1"][~off]).any())
