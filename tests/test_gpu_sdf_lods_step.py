"""GPU: the fused all-LOD octree SDF training step (wisp_sdf_lods_train_step, csrc/spc_grad.hip) against the float64 restatement of
tests/sdf_lods_step_ref.py, element for element, and what is built on it: SDFTrainStep(only_last=False, fused_lods=True), eager and
graph-captured, and scripts/train_nglod.py --all-lods --fused-step.
Exact inputs (the reference file proves per case that no product and no partial sum of any LOD rounds, in any order of addition): the
loss [1 + L] / [1 + 2L] and every gradient, ADDED to pre-filled buffers, equal float64 BIT FOR BIT.  One level is the existing steps,
bit for bit on generic inputs.  Generic batch sizes stay inside a bound derived per element from its own terms.
Every measured figure is appended to the file WISP_SDF_LODS_STEP_MARGINS names (profiles/sdf_lods_step_test_margins.jsonl)."""
import copy
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import sdf_lods_step_ref as R
import sdf_step_exact_ref as X
import test_gpu_sdf_step_exact as E

pytestmark = pytest.mark.gpu
DEV = E.DEV
GRADS = E.GRADS
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def record(name, **values):
    path = os.environ.get("WISP_SDF_LODS_STEP_MARGINS")
    if path:
        with open(path, "a") as f:
            f.write(json.dumps(dict(name=name, **{k: (v if isinstance(v, (int, str, list, bool)) else float(v)) for k, v in values.items()})) + "\n")


def n_loss(case):
    return 1 + (2 if case["tex"] else 1) * len(case["levels"])


def run_lods(case, before, gts=None, rgb=None, calls=1, w_sdf=None, w_rgb=None):
    """`calls` launches on buffers holding `before` -> dict of host tensors: the loss and the buffers afterwards"""
    import wisp._C as C
    i = E._inputs(case, gts, rgb)
    d_sdf, d_rgb = R.default_weights(case)
    w_sdf = w_sdf or case.get("w_sdf") or d_sdf
    w_rgb = (w_rgb or case.get("w_rgb") or d_rgb) if case["tex"] else None
    bufs = {k: before[k].to(DEV).contiguous() for k in GRADS}
    tabs = [t.to(DEV).contiguous() for t in before["tables"]]
    for _ in range(calls):
        loss = C.sdf_lods_train_step(i["coords"], i["gts"], i["rgb"] if case["tex"] else None, i["octree"], i["exsum"], i["points"],
                                     i["trinkets"], i["feats"], i["levels"], case["half_round"], case["pos_input"], w_sdf, w_rgb,
                                     i["w1"], i["b1"], i["w2"], i["b2"], tabs, bufs["w1"], bufs["b1"], bufs["w2"], bufs["b2"])
    assert loss.shape == (n_loss(case),) and loss.dtype == torch.float32
    return dict(loss=loss.cpu(), tables=[t.cpu() for t in tabs], **{k: v.cpu() for k, v in bufs.items()})


def check_exact(case, tag="exact"):
    before = E.prefill(case)
    got = run_lods(case, before)
    E.assert_bits(case, got, before)
    rep = case["report"]
    record(tag, tex=int(case["tex"]), levels=str(case["levels"]), n=case["n"], hidden=case["hidden"], b=case["b"], align=case["align"],
           half_round=int(case["half_round"]), pos_input=case["pos_input"], bits_used=max(rep["spans"].values()), relu_edge=rep["edge"],
           distinct_preds=rep["distinct_preds"], table_entries_moved=sum(int((w != 0).sum()) for w in case["want"]["tables"]))
    return got, before


LISTS = list(range(len(R.LEVEL_LISTS)))


# ------------------------------------------------------------------------------------------------ exact: level lists x n
@pytest.mark.parametrize("n", R.NS)
@pytest.mark.parametrize("li", LISTS, ids=[f"{t}{len(l)}" for t, l in R.LEVEL_LISTS])
@pytest.mark.parametrize("tex", [0, 1])
def test_step_equals_float64_bit_for_bit(tex, li, n):
    """1, 2, 3, 6, 8 and 9 levels (16, 8, 5, 2, 2 and 1 samples per pass; 0, 0, 1, 4, 0 and 7 idle groups) at n = 1, 2, 16, 64, 512:
    tail passes (n = 1 at 6 levels, n = 16 at 3), samples outside the cube and in empty cells; the textured step alternates its
    input layout.  No listed shape was refused by check_exact_lods, so none was lowered."""
    tree, levels = R.LEVEL_LISTS[li]
    assert (lambda s: (s["spb"], s["idle_groups"]))(R.launch_shape(len(levels), n)) == R.COVERAGE[len(levels)]
    kw = dict(tex=True, pos_input=(li + n) % 2) if tex else {}
    check_exact(R.exact_lods_case(tree, levels, n, 24 if tex else 16, **kw))


def test_second_grid_stride_pass():
    """9 levels, n = 2048: 1 sample per pass, 1024 workgroups, every one makes two passes.  (The plain field: with colours the exact
    checker refuses this n at every rung - the weighted total of the loss needs 24.8 bits; the textured second pass is in the
    bounded test at n = 2049 over six levels.)"""
    tree, levels, n = R.TWO_PASS
    shape = R.launch_shape(len(levels), n)
    assert shape["grid"] == X.GRID_CAP and shape["second_pass_all"]
    check_exact(R.exact_lods_case(tree, levels, n, 16), "exact two passes")


# ------------------------------------------------------------------------------------------------ exact: the decoder
@pytest.mark.parametrize("hidden", R.HIDDENS)
@pytest.mark.parametrize("tex,pos", [(0, 1), (1, 1), (1, 0)])
def test_hidden_widths(tex, pos, hidden):
    """1 unit, 17 (no multiple of 16), 128 and ST_MAX_HIDDEN = 256 (dynamic LDS above 64 KB), on 3 levels: 5 samples per pass"""
    check_exact(R.exact_lods_case("small", (3, 4, 5), 64, hidden, tex=bool(tex), pos_input=pos))


@pytest.mark.parametrize("n", [16, 512])
@pytest.mark.parametrize("levels", [(5,), (3, 4, 5), (0, 1, 2, 3, 4, 5)])
@pytest.mark.parametrize("tex,pos", [(0, 1), (1, 1), (1, 0)])
def test_half_round(tex, pos, levels, n):
    check_exact(R.exact_lods_case("small", levels, n, 24, tex=bool(tex), pos_input=pos, half_round=True))
    check_exact(R.exact_lods_case("small", levels, n, 24, tex=bool(tex), pos_input=pos, half_round=False))


@pytest.mark.parametrize("modes", [("half",) * 3, ("low",) * 3, ("high",) * 3], ids="-".join)
def test_colour_modes(modes):
    case = R.exact_lods_case("small", (2, 3, 4, 5), 64, 24, tex=True, pos_input=1, modes=modes)
    got, before = check_exact(case)
    L = len(case["levels"])
    for o, m in enumerate(modes):                      # a saturated colour has no gradient: its rows keep the pre-filled bits
        if m != "half":
            assert torch.equal(got["w2"][o], before["w2"][o]) and torch.equal(got["b2"][o], before["b2"][o])
        else:
            assert not torch.equal(got["w2"][o], before["w2"][o])
    assert all(float(v) > 0 for v in got["loss"][1 + L:])


@pytest.mark.parametrize("tex", [0, 1])
def test_the_relu_edge_unit(tex):
    """samples whose pre-activation of the edge unit is exactly 0 at the finest LOD with a gradient to lose: the backward selects"""
    case = R.exact_lods_case("small", (3, 4, 5), 64, 24, tex=bool(tex))
    assert case["report"]["edge"] >= 1
    check_exact(case)


@pytest.mark.parametrize("tex", [0, 1])
def test_a_batch_that_misses_every_cell(tex):
    case = R.exact_lods_case("deep", (8, 9, 10), 64, 24, tex=bool(tex), all_miss=True)
    assert bool((case["chain"] < 0).all())
    got, before = check_exact(case)
    for g, b in zip(got["tables"], before["tables"]):
        assert torch.equal(g, b)
    assert torch.equal(got["w1"][:, 3:], before["w1"][:, 3:]) and not torch.equal(got["w1"][:, :3], before["w1"][:, :3])


@pytest.mark.parametrize("tex", [0, 1])
def test_a_second_call_adds_the_same_amounts_again(tex):
    case = R.exact_lods_case("small", (2, 3, 4, 5), 64, 24, tex=bool(tex))
    before = E.prefill(case)
    got = run_lods(case, before, calls=2)
    E.assert_bits(case, got, before, times=2)


# ------------------------------------------------------------------------------------------------ scratch bounds
PAD = 4096
SENTINEL = 0xA5


def _raw_call(case, before, scratch_ptr, need, w_sdf, w_rgb):
    """the C entry point itself on an explicit scratch -> (rc, loss, bufs, tabs)"""
    import wisp._C as C
    i = E._inputs(case)
    L, H, tex = len(case["levels"]), case["w1"].shape[0], case["tex"]
    bufs = {k: before[k].to(DEV).contiguous() for k in GRADS}
    tabs = [t.to(DEV).contiguous() for t in before["tables"]]
    rarr, rptr = C._host_i64([f.shape[0] for f in i["feats"]])
    ws = C._spc_bwd_workspace(torch.device(DEV), int(rarr.sum()), X.C)
    farr, fptr = C._ptr_array(i["feats"])
    garr, gptr = C._ptr_array(tabs)
    larr, lptr = C._host_i32(i["levels"])
    loss = torch.empty(n_loss(case), dtype=torch.float32, device=DEV)
    ws_arr = (ctypes.c_float * L)(*w_sdf)
    wr_arr = (ctypes.c_float * L)(*w_rgb) if tex else None
    p = C._p
    rc = C._cdll.wisp_sdf_lods_train_step(
        p(i["coords"]), p(i["gts"]), p(i["rgb"]) if tex else None, case["n"], p(i["octree"]), p(i["exsum"]), p(i["points"]), p(i["trinkets"]),
        fptr, lptr, rptr, L, X.C, int(case["half_round"]), 4 if tex else 1, case["pos_input"], ctypes.cast(ws_arr, ctypes.c_void_p),
        ctypes.cast(wr_arr, ctypes.c_void_p) if tex else None, p(i["w1"]), p(i["b1"]), p(i["w2"]), p(i["b2"]), H, gptr, p(bufs["w1"]),
        p(bufs["b1"]), p(bufs["w2"]), p(bufs["b2"]), p(loss), scratch_ptr, need, p(ws), ws.numel(), C._stream())
    torch.cuda.synchronize()
    return rc, loss, bufs, tabs


@pytest.mark.parametrize("tex,li,n,hidden", [(0, 2, 37, 17), (1, 3, 64, 24), (0, 5, 16, 16)])
def test_nothing_is_written_behind_the_declared_scratch_size(tex, li, n, hidden):
    """a scratch of exactly wisp_sdf_lods_train_scratch_bytes inside a larger allocation filled with a sentinel: the bytes before and
    behind it are unchanged, the results those of the cached-scratch call"""
    import wisp._C as C
    tree, levels = R.LEVEL_LISTS[li]
    big = R.exact_lods_case(tree, levels, 64, hidden, tex=bool(tex))
    case = big if n == 64 else R.inexact_lods_case(big, n)
    before = E.prefill(case)
    cached = run_lods(case, before)
    need = int(C.lib.wisp_sdf_lods_train_scratch_bytes(n, len(levels), X.C, hidden, 4 if tex else 1, case["pos_input"]))
    assert need > 0
    arena = torch.full((need + 2 * PAD,), SENTINEL, dtype=torch.uint8, device=DEV)
    w_sdf, w_rgb = R.default_weights(case)
    rc, loss, bufs, tabs = _raw_call(case, before, ctypes.c_void_p(arena.data_ptr() + PAD), need, w_sdf, w_rgb)
    assert rc == 0, C.lib.wisp_last_error()
    host = arena.cpu()
    assert bool((host[:PAD] == SENTINEL).all()) and bool((host[PAD + need:] == SENTINEL).all())
    assert not bool((host[PAD:PAD + need] == SENTINEL).all())
    assert torch.equal(loss.cpu(), cached["loss"])
    for k in GRADS:
        assert torch.equal(bufs[k].cpu(), cached[k]), k
    assert all(torch.equal(a.cpu(), b) for a, b in zip(tabs, cached["tables"]))


# ------------------------------------------------------------------------------------------------ one level is the existing step
def _generic_case(tex, pos, n, levels, hidden, seed):
    """fp32 inputs with nothing exact about them, in the layout of an exact case"""
    base = X.exact_case("small", levels, 64, 24, tex=bool(tex), pos_input=pos)
    rng = np.random.default_rng(seed)
    tr = base["tree"]
    pts = tr.level_points(levels[-1])
    c = ((pts[rng.integers(0, pts.shape[0], n)] + rng.uniform(0.02, 0.98, (n, 3))) / 2.0 ** (levels[-1] - 1) - 1).astype(np.float32)
    c[4::9] = rng.uniform(-1.2, 1.2, (c[4::9].shape[0], 3))             # some outside every cell / the unit cube (never sample 0)
    in_dim = (3 if pos else 0) + X.C
    rows = 4 if tex else 1
    f32 = lambda a: torch.from_numpy(np.asarray(a, dtype=np.float32))
    return dict(base, n=n, N=n, coords=f32(c), gts=f32(rng.normal(size=n) * 0.1), rgb_gts=f32(rng.uniform(size=(n, 3))),
                tables=[f32(rng.normal(size=(tr.rows(l), X.C)) * 0.3) for l in levels],
                w1=f32(rng.normal(size=(hidden, in_dim)) * 0.4), b1=f32(rng.normal(size=hidden) * 0.1),
                w2=f32(rng.normal(size=(rows, hidden)) * 0.3), b2=f32(rng.normal(size=rows) * 0.1), hidden=hidden, half_round=False)


@pytest.mark.parametrize("n", [1, 37, 512, 5000])
@pytest.mark.parametrize("tex,pos", [(0, 1), (1, 1), (1, 0)])
def test_one_level_with_weight_one_is_the_existing_step_bit_for_bit(tex, pos, n):
    """L = 1, weights 1, generic fp32 inputs: loss and every gradient equal wisp_sdf_train_step's / wisp_sdf_tex_train_step's bits;
    the new loss [1 + L] / [1 + 2L] maps onto the old [1] / [3] by index"""
    case = _generic_case(tex, pos, n, (5,), 128 if n != 37 else 17, 900 + n)
    before = E.prefill(case)
    old = E.run_step(case, before)
    new = run_lods(case, before, w_sdf=[1.0], w_rgb=[1.0])
    # old [1] = {total / n} is new[0] (new[1] = S_0 has no counterpart); old [3] = {total / n, S, R} is new [1 + 2] entry for entry
    assert new["loss"].shape == ((3,) if tex else (2,))
    assert torch.equal(new["loss"][:old["loss"].numel()], old["loss"]), (new["loss"].tolist(), old["loss"].tolist())
    assert float(new["loss"][1]) > 0
    for k in GRADS:
        assert torch.equal(new[k], old[k]) and not torch.equal(new[k], before[k]), k
    assert torch.equal(new["tables"][0], old["tables"][0]) and not torch.equal(new["tables"][0], before["tables"][0])


# ------------------------------------------------------------------------------------------------ forward
@pytest.mark.parametrize("tex", [0, 1])
def test_forward_of_every_lod_is_the_querys_value_bit_for_bit(tex):
    """n = 1, target 0, a six-level field: loss[1 + k] is the fp32 square of wisp_sdf_query's distance on the first k + 1 levels
    (lod_idx = k), for every k"""
    import wisp._C as C
    case = R.exact_lods_case("small", (0, 1, 2, 3, 4, 5), 1, 24, tex=bool(tex))
    got = run_lods(case, E.prefill(case, zero=True), gts=torch.zeros(1))
    i = E._inputs(case)
    distinct = set()
    for k in range(6):
        fld = dict(E.dev_tree(case), feats=i["feats"][:k + 1], levels=i["levels"][:k + 1], half_round=False, w1=i["w1"], b1=i["b1"],
                   w2=i["w2"], b2=i["b2"])
        v = np.float32(C.sdf_query(i["coords"], fld).cpu().numpy()[0, -1])
        assert float(v) == float(case["want"]["pred"][k][0])
        assert np.float32(got["loss"][1 + k].item()) == v * v, (k, got["loss"][1 + k].item(), float(v * v))
        distinct.add(float(v))
    assert len(distinct) >= 4


# ------------------------------------------------------------------------------------------------ weights
@pytest.mark.parametrize("k", [0, 2, 3])
def test_doubling_one_lods_weight_adds_exactly_that_lods_contribution(k):
    levels = (2, 3, 4, 5)
    one = R.exact_lods_case("small", levels, 64, 16)
    w = [1.0] * 4
    w[k] = 2.0
    two = R.exact_lods_case("small", levels, 64, 16, w_sdf=tuple(w))
    assert two["align"] == one["align"] and two["b"] == one["b"] and torch.equal(two["gts"], one["gts"])
    before = E.prefill(one)
    a, b = run_lods(one, before), run_lods(two, before)
    E.assert_bits(one, a, before)
    E.assert_bits(two, b, before)
    add = one["want"]["per_lod"][k]
    for name in GRADS:
        assert torch.equal(b[name].double() - a[name].double(), add[name].reshape(a[name].shape)), name
        assert bool(add[name].any())
    for l, (tb, ta) in enumerate(zip(b["tables"], a["tables"])):
        assert torch.equal(tb.double() - ta.double(), add["tables"][l]), l
        assert bool(add["tables"][l].any()) == (l <= k)
    assert float(b["loss"][1 + k]) == float(a["loss"][1 + k])             # S_k itself carries no weight


# ------------------------------------------------------------------------------------------------ generic batch sizes
def check_bounded(case, tag):
    before = E.prefill(case)
    got = run_lods(case, before)
    again = run_lods(case, before)
    assert torch.equal(got["loss"], again["loss"]) and all(torch.equal(got[k], again[k]) for k in GRADS)        # bitwise repeatable
    assert all(torch.equal(a, b) for a, b in zip(got["tables"], again["tables"]))
    bounds = R.derived_bounds(case, before)
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
    assert any(v > 0 for v in worst.values())


@pytest.mark.parametrize("n", R.INEXACT_NS)
@pytest.mark.parametrize("tex,pos", [(0, 1), (1, 1), (1, 0)])
def test_sums_stay_within_the_derived_bound_at_other_batch_sizes(tex, pos, n):
    """n = 37, 513 over three levels: fl(1 / n) is no power of two, the sums round - every element within the bound of
    sdf_lods_step_ref.derived_bounds; two runs give the same bits"""
    size = 64 if n < 64 else 1024
    case = R.inexact_lods_case(R.forward_exact_lods_case("small", (3, 4, 5), size, 24, tex=bool(tex), pos_input=pos), n)
    check_bounded(case, f"tex{tex} pos{pos} n{n}")


@pytest.mark.parametrize("tex", [0, 1])
def test_sums_stay_within_the_derived_bound_at_2049_over_six_levels(tex):
    """2 samples per pass, 1024 workgroups, one of them makes a second pass - with a single sample in it"""
    tree, levels, n = R.INEXACT_BIG
    assert R.launch_shape(len(levels), n)["max_passes"] == 2
    case = R.inexact_lods_case(R.forward_exact_lods_case(tree, levels, 4096, 16, tex=bool(tex)), n)
    check_bounded(case, f"tex{tex} six levels n{n}")


# ------------------------------------------------------------------------------------------------ a non-finite target
@pytest.mark.parametrize("tex", [0, 1])
def test_one_infinite_target(tex):
    """one target of +inf: every element the float64 reference keeps finite is bit-equal (units that are off for that sample pass 0
    on at every LOD, rows it does not touch), every element the reference makes non-finite is non-finite: the scatter's
    non-finite path"""
    case = R.exact_lods_case("small", (3, 4, 5), 16, 24, tex=bool(tex))
    gts = case["gts"].clone()
    gts[3] = float("inf")
    want = R.lods_reference(case, gts=gts)
    before = E.prefill(case)
    got = run_lods(case, before, gts=gts)
    pairs = [("loss", got["loss"].double(), want["loss"])]
    pairs += [(k, got[k].double(), before[k].double() + want[k].reshape(before[k].shape)) for k in GRADS]
    pairs += [(f"table{li}", g.double(), b.double() + w) for li, (g, b, w) in enumerate(zip(got["tables"], before["tables"], want["tables"]))]
    finite_seen = 0
    for name, g, w in pairs:
        fin = torch.isfinite(w)
        assert not bool(torch.isfinite(g[~fin]).any()), (name, "finite where float64 is not")
        bad = g[fin] != w[fin]
        assert not bool(bad.any()), (name, "differs where float64 is finite", int(bad.sum()), g[fin][bad][:4].tolist(), w[fin][bad][:4].tolist())
        if name != "loss":
            finite_seen += int(fin.sum()) if not bool(fin.all()) else 0
    assert not bool(torch.isfinite(want["loss"][0])) and finite_seen > 0
    off = torch.stack([q["a"][3] <= 0 for q in R.lods_parts(case, gts=gts)["lods"]]).all(0)
    assert bool(off.any()) and bool(torch.isfinite(want["b1"][off]).all())


# ------------------------------------------------------------------------------------------------ SDFTrainStep
def _random_cells(seed):
    from wisp.accelstructs import OctreeAS
    rng = np.random.default_rng(seed)
    P = rng.integers(0, 32, size=(4000, 3))
    return rng, P, OctreeAS.from_quantized_points(torch.from_numpy(P.astype(np.int16)).to(DEV), 5)


def _field(blas, tex, pos=True, lods=4, hidden=128, seed=7, std=0.05):
    from wisp.models.grids import OctreeGrid
    from wisp.models.nefs import NeuralSDF
    from wisp.models.nefs.neural_sdf_tex import NeuralSDFTex
    torch.manual_seed(seed)
    grid = OctreeGrid(blas, feature_dim=16, num_lods=lods, multiscale_type='sum', feature_std=std)
    if tex:
        return NeuralSDFTex(grid, embedder_type='identity' if pos else 'none', hidden_dim=hidden, num_layers=1).to(DEV)
    return NeuralSDF(grid, pos_embedder='none', position_input=True, hidden_dim=hidden, num_layers=1).to(DEV)


def _batch(rng, P, n):
    c = ((P[rng.integers(0, P.shape[0], n)] + rng.uniform(0.02, 0.98, (n, 3))) / 16 - 1).astype(np.float32)
    c[::11] = rng.uniform(-1.2, 1.2, (c[::11].shape[0], 3))
    to = lambda a: torch.from_numpy(a).to(DEV)
    return to(c), to(rng.normal(size=(n, 1)).astype(np.float32) * 0.1), to(rng.uniform(size=(n, 3)).astype(np.float32))


@pytest.mark.parametrize("tex,pos,batch", [(0, True, 512), (1, True, 512), (1, False, 37)])
def test_fused_all_lod_step_equals_the_modular_launches(tex, pos, batch):
    """SDFTrainStep(only_last=False, fused_lods=True) against SDFTrainStep(only_last=False) (one query + decoder per LOD through
    autograd) from the same state: same loss, same gradient in every parameter, within the tolerances the one-LOD fused steps are
    held to against their modular launches; last_l2 / last_rgb are the finest LOD's sums = loss[L], loss[2L]; same bits again"""
    from wisp.trainers import SDFTrainStep
    rng, P, blas = _random_cells(340 + batch)
    nef_a = _field(blas, tex, pos)
    nef_b = copy.deepcopy(nef_a)
    fused = SDFTrainStep(nef_a, lr=1e-3, eps=1e-15, grid_lr_weight=2.0, only_last=False, fused_lods=True)
    modular = SDFTrainStep(nef_b, lr=1e-3, eps=1e-15, grid_lr_weight=2.0, only_last=False)
    assert fused._fused_field() is not None and fused._fused_field()["lods_loss"] and modular._fused_field() is None
    coords, gts, col = _batch(rng, P, batch)
    args = (coords, gts, col) if tex else (coords, gts)
    la, lb = fused._forward_backward(*args), modular._forward_backward(*args)
    tag = f"tex={tex} pos={int(pos)} B={batch}"
    err = abs(float(la) - float(lb))
    record("fused vs modular", case=tag, loss_err=err, loss=float(lb))
    assert err <= 1e-5 * max(1.0, abs(float(lb))), (tag, float(la), float(lb))
    if tex:
        assert abs(float(fused.last_l2) - float(modular.last_l2)) <= 1e-5 * max(1.0, abs(float(modular.last_l2)))
        assert abs(float(fused.last_rgb) - float(modular.last_rgb)) <= 1e-5 * max(1.0, abs(float(modular.last_rgb)))
    worst = 0.0
    for (n1, p1), (n2, p2) in zip(nef_a.named_parameters(), nef_b.named_parameters()):
        sc = max(float(p2.grad.abs().max()), 1e-12)
        e = float((p1.grad - p2.grad).abs().max())
        worst = max(worst, e / (2e-5 * sc))
        assert e <= 2e-5 * sc, (tag, n1, e, sc)
        assert float(p2.grad.abs().max()) > 0
    record("fused vs modular grads", case=tag, worst_error_over_bound=worst)
    ga, l2, lr = fused.flat.grad.clone(), fused.last_l2, fused.last_rgb
    fused.flat.grad.zero_()
    la2 = fused._forward_backward(*args)
    assert torch.equal(fused.flat.grad, ga) and float(la2) == float(la)
    if tex:
        assert torch.equal(fused.last_l2, l2) and torch.equal(fused.last_rgb, lr)


@pytest.mark.parametrize("tex", [0, 1])
def test_last_l2_and_last_rgb_are_views_of_the_loss_tensor(tex, monkeypatch):
    import wisp._C as C
    from wisp.trainers import SDFTrainStep
    rng, P, blas = _random_cells(77)
    nef = _field(blas, tex, lods=3, hidden=32)
    step = SDFTrainStep(nef, only_last=False, fused_lods=True)
    seen = []
    inner = C.sdf_lods_train_step
    monkeypatch.setattr(C, "sdf_lods_train_step", lambda *a, **k: seen.append(inner(*a, **k)) or seen[-1])
    coords, gts, col = _batch(rng, P, 64)
    loss = step._forward_backward(*((coords, gts, col) if tex else (coords, gts)))
    out = seen[0]
    assert out.shape == ((7,) if tex else (4,)) and loss.data_ptr() == out.data_ptr()
    if tex:
        assert step.last_l2.data_ptr() == out[3].data_ptr() and step.last_rgb.data_ptr() == out[6].data_ptr()
        assert float(step.last_l2) == float(out[3]) and float(step.last_rgb) == float(out[6])
        total = sum(float(out[1 + k]) for k in range(3)) + sum((3 - k) * float(out[4 + k]) for k in range(3))
        assert abs(float(out[0]) - total / 64) <= 1e-5 * max(1.0, total / 64)


@pytest.mark.parametrize("tex", [0, 1])
def test_graph_replay_is_the_eager_step_bit_for_bit(tex):
    from wisp.trainers import SDFTrainStep
    rng, P, blas = _random_cells(78)
    nef_a = _field(blas, tex, lods=4, hidden=64)
    nef_b = copy.deepcopy(nef_a)
    eager = SDFTrainStep(nef_a, lr=1e-3, eps=1e-15, only_last=False, fused_lods=True)
    graph = SDFTrainStep(nef_b, lr=1e-3, eps=1e-15, only_last=False, fused_lods=True).capture(512)
    assert graph._fused_field() is not None and graph._fused_field()["lods_loss"]
    start = {n: p.detach().clone() for n, p in nef_b.named_parameters()}
    for it in range(4):
        coords, gts, col = _batch(rng, P, 512)
        args = (coords, gts, col) if tex else (coords, gts)
        la, lb = eager.step(*args), graph.step(*args)
        assert float(la) == float(lb), it
        if tex:
            assert float(eager.last_l2) == float(graph.last_l2) and float(eager.last_rgb) == float(graph.last_rgb)
    moved = 0.0
    for (n1, p1), (n2, p2) in zip(nef_a.named_parameters(), nef_b.named_parameters()):
        assert torch.equal(p1.detach(), p2.detach()), n1
        moved = max(moved, float((p2.detach() - start[n2]).abs().max()))
    assert moved > 1e-3


def test_thirty_adam_steps_stay_as_close_to_float64_as_the_modular_steps():
    """30 Adam steps (lr 1e-3, grid x 2, eps 1e-15) on one batch: the fused all-LOD trainer, the modular all-LOD trainer, and torch
    autograd + torch.optim.Adam in float64 over the CPU oracle's lookup and decoder with the reference's loop.  The distance of a
    trajectory from float64 is the Euclidean norm of the difference of all parameters after the 30 steps (the largest and the median
    difference are recorded beside it).  The fused distance may be at most twice the modular one: the allowance the fused-step
    tests use for a different but equally valid rounding order.  Both are measured here and recorded."""
    from oracle import nerf as onerf, octree_grid as og, spc as ospc
    from wisp.accelstructs import OctreeAS
    from wisp.trainers import SDFTrainStep
    rng = np.random.default_rng(31)
    P = np.unique(rng.integers(0, 16, size=(600, 3)), axis=0)
    blas = OctreeAS.from_quantized_points(torch.from_numpy(P.astype(np.int16)).to(DEV), 4)
    oblas = onerf.OracleBLAS(ospc.points_to_octree(P, 4))
    pd, pyd = ospc.make_dual(oblas.points, oblas.pyramid)
    tr, _ = ospc.make_trinkets(oblas.points, oblas.pyramid, pd, pyd)
    L, H, B = 3, 32, 256
    nef_f = _field(blas, 0, lods=L, hidden=H, seed=3)
    nef_f.grid.half_features = False
    nef_m = copy.deepcopy(nef_f)
    c = ((P[rng.integers(0, P.shape[0], B)] + rng.uniform(0.05, 0.95, (B, 3))) / 8 - 1).astype(np.float32)
    gt = (np.linalg.norm(c, axis=1, keepdims=True) - 0.5).astype(np.float32)
    feats = [f.detach().cpu().double().clone().requires_grad_(True) for f in nef_f.grid.features[:L]]
    dec = onerf.OracleDecoder(3 + 16, 1, H, 1, True).double()
    dec.load_state_dict({k: v.detach().cpu().double() for k, v in nef_f.decoder.state_dict().items()})
    opt = torch.optim.Adam([{"params": list(dec.parameters()), "lr": 1e-3}, {"params": feats, "lr": 2e-3}], eps=1e-15)
    active = list(nef_f.grid.active_lods[:L])
    c64, gt64 = torch.from_numpy(c), torch.from_numpy(gt).double()
    for _ in range(30):
        opt.zero_grad()
        loss = 0.0
        for k in range(L):
            f = og.octree_grid_interpolate(oblas, tr, feats, c64, k, nef_f.grid.base_lod, active, 'sum', 16, False)
            loss = loss + ((dec(torch.cat([c64.double(), f.double()], -1)) - gt64) ** 2).sum()
        (loss / B).backward()
        opt.step()
    fused = SDFTrainStep(nef_f, lr=1e-3, eps=1e-15, grid_lr_weight=2.0, only_last=False, fused_lods=True)
    modular = SDFTrainStep(nef_m, lr=1e-3, eps=1e-15, grid_lr_weight=2.0, only_last=False)
    assert fused._fused_field() is not None and modular._fused_field() is None
    cd, gd = torch.from_numpy(c).to(DEV), torch.from_numpy(gt).to(DEV)
    for _ in range(30):
        lf, lm = fused.step(cd, gd), modular.step(cd, gd)
    want = [p.detach() for p in feats] + [dec.layers[0].weight.detach(), dec.layers[0].bias.detach(), dec.lout.weight.detach(), dec.lout.bias.detach()]

    def distance(nef):
        got = list(nef.grid.features[:L]) + [nef.decoder.layers[0].weight, nef.decoder.layers[0].bias, nef.decoder.lout.weight, nef.decoder.lout.bias]
        d = torch.cat([(g.detach().cpu().double() - w).reshape(-1) for g, w in zip(got, want)])
        return float(d.norm()), float(d.abs().max()), float(d.abs().median())
    (df, df_max, df_med), (dm, dm_max, dm_med) = distance(nef_f), distance(nef_m)
    record("thirty adam steps", fused_l2=df, modular_l2=dm, fused_max=df_max, modular_max=dm_max, fused_median=df_med, modular_median=dm_med,
           loss_fused=float(lf), loss_modular=float(lm), loss_float64=float(loss / B))
    print(f"30 Adam steps: distance from float64 fused {df:.3e} (max {df_max:.3e}), modular {dm:.3e} (max {dm_max:.3e})")
    assert abs(float(lf) - float(loss / B)) <= 1e-3 * max(1.0, float(loss / B))
    assert df <= 2.0 * dm, (df, dm)


# ------------------------------------------------------------------------------------------------ end to end
def test_train_nglod_script_trains_every_lod_through_the_fused_step(tmp_path):
    """scripts/train_nglod.py --all-lods --fused-step on the procedural torus: the field takes the all-LOD step and every LOD's IoU
    rises.  The same run with --fused-step alone (the finest LOD in the loss: the state of things without the all-LOD step) is
    recorded beside it; only its finest LOD is expected to be comparable, and no threshold is put on its coarse ones."""
    recs = {}
    for name, extra in (("all_lods", ["--all-lods"]), ("only_last", [])):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "train_nglod.py"), "--write-test-mesh", str(tmp_path / "mesh"),
                            "--level", "5", "--num-lods", "3", "--num-samples", "8000", "--mesh-samples", "200000", "--epochs", "4",
                            "--fused-step", "--seed", "0", "--size", "32", "32", "--out-dir", str(tmp_path / name)] + extra,
                           capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-3000:]
        recs[name] = json.loads(r.stdout.strip().splitlines()[-1])
    a, o = recs["all_lods"], recs["only_last"]
    record("script", all_lods_before=a["iou_lods_before"], all_lods_after=a["iou_lods_after"], only_last_before=o["iou_lods_before"],
           only_last_after=o["iou_lods_after"], seconds_all_lods=a["seconds"], seconds_only_last=o["seconds"])
    assert a["all_lods"] is True and a["fused_lods_step"] is True and a["fused_step"] is True
    assert o["all_lods"] is False and o["fused_lods_step"] is False
    assert len(a["iou_lods_after"]) == 3 == len(a["iou_lods_before"]) == len(o["iou_lods_after"])
    for k in range(3):
        assert a["iou_lods_after"][k] > a["iou_lods_before"][k], (k, a["iou_lods_before"], a["iou_lods_after"])
    assert a["iou_after"] == a["iou_lods_after"][-1] and o["iou_after"] == o["iou_lods_after"][-1]
