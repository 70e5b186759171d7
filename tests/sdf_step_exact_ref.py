"""float64 restatement of the two fused octree SDF training steps (csrc/spc_grad.hip: wisp_sdf_train_step = sdf_train_kernel +
sdf_train_reduce_kernel + the wide scatter + finalize, and wisp_sdf_tex_train_step), a generator of exactly representable training
cases and the checker that proves them exact.  Test infrastructure only; host only (numpy + torch CPU).  The tree, the sample
coordinates, the cell chain and the trilinear weights are those of tests/spc_exact_ref.py (Tree, make_case, weights): nothing of the
octree walk is restated here.

The gradients are written out, not taken from autograd (tests/hash_sdf_step_ref.step_reference is the model).  With
x = [position,] sum_l blend_l, a = W1 x + b1, h = relu(a):
  one output    pred = w2 . h + b2, g = fl32(2 (pred - gt) inv_n);  d b2 = sum g, d w2 = h^T g, ga = [a > 0] g w2
  four outputs  y = W2 h + b2, rgb = sigmoid(y[0:3]), g_o = fl32(2 (rgb_o - rgb_gt_o) rgb_o (1 - rgb_o) inv_n), g_3 = fl32(2 (y_3 - gt)
                inv_n);  d b2 = sum g, d W2 = g^T h, ga[h] = [a_h > 0] sum_o W2[o][h] g_o;
                loss[3] = {(distance sum + colour sum) inv_n, distance sum, colour sum} (sdf_tex_train_reduce_kernel)
  both          d b1 = sum ga, d W1 = ga^T x, d features = ga W1[:, feature columns], and the table gradient of every level is a float64
                scatter-add of weight * d features over the eight corner rows of the level's cell; a sample that misses a level's
                cell adds nothing there, its d features still come from the levels it hit.
[a > 0] SELECTS (torch.relu's backward): a masked unit passes exactly 0 on, whatever g is - also an infinite g.
inv_n is the fp32 value fl(1 / n) taken into float64, g is rounded to fp32 once: what `2.0f * diff * inv_batch` computes when 2 diff is
exact.  half_round: every table value is rounded through fp16 before the blend and every level's blend before the sum over levels.
The sigmoid is taken in fp32 (the colour modes below make expf exactly 1, 0 or +inf there; float64 would keep 2.6e-56 of a colour).

Exact cases.  Samples sit in cells of the finest active level at offsets k / 2^b per axis (make_case); with b = 0 in cells whose
coordinates are multiples of 2^align, which leaves a level d levels coarser max(0, d - align) fraction bits per axis.  Tables hold
integers in [-1, 1] (half_round: a share of them plus 2^-13, which the fp16 rounding takes away again), W1 three entries of -1 / 1
per row, w2 / W2 -1 / 0 / 1 with at most 16 non-zero entries per row, the biases small integers, the target of a sample is its own
float64 prediction plus a multiple of 1/4 in [-1, 1], n is a power of two.  check_exact_step then finds ONE quantum per stage and
output (the largest power of two that divides every term and the pre-filled value) and asserts that the absolute values of all
terms sum to fewer than 2^24 quanta: every partial sum in any order of addition is an fp32 value, so a kernel must equal the float64
result BIT FOR BIT.  A failing assertion there blames the inputs, not the kernel.  exact_case walks a fixed list of (b, align) from the
richest to the plainest and takes the first the checker accepts.
"""
import numpy as np
import torch

import spc_exact_ref as S

F64 = torch.float64
C = 16                                 # feature channels: the fused steps are built for 16 (ST_GROUP)
ST_GROUPS = 16                         # spc_grad.hip: lane groups of a workgroup = (sample, level) pairs of one pass
GRID_CAP = 1024                        # spc_grad.hip st_grid: workgroups at most
PREFILL_MAX = 2.0                      # |value| a gradient buffer may be pre-filled with (multiples of 1/2)
EDGE_UNIT = 0                          # the hidden unit whose pre-activation is exactly 0 on part of the samples
COLOUR_MODES = ("half", "low", "high")     # per colour channel: expf exactly 1 / +inf / 0 (make_decoder)
SAT_BIAS = 128.0
ZERO_CAP = 0.15


# ---------------------------------------------------------------------------------------------------- trees
def _lattice(level, align, keep):
    a = np.arange(0, 2 ** level, 2 ** align)
    P = np.stack(np.meshgrid(a, a, a, indexing='ij'), -1).reshape(-1, 3)
    idx = (P >> align).sum(1)
    return P[idx % 4 != 3] if keep else P[idx % 4 == 3]


_trees = {}


def tree(name):
    """'small': level 5, 3000 random cells and three quarters of the cells whose coordinates are multiples of 4;  'deep': level 10,
    200 random cells and three quarters of the cells whose coordinates are multiples of 128 (a few hundred cells per level)"""
    if name not in _trees:
        _trees[name] = S.Tree(5, 3000, 401, extra=_lattice(5, 2, True)) if name == "small" else S.Tree(10, 200, 402, extra=_lattice(10, 7, True))
    return _trees[name]


# ---------------------------------------------------------------------------------------------------- what a launch reaches
def launch_shape(num_lods, n):
    """restated from sdf_train_kernel / st_grid: samples per pass, workgroups, and what the (levels, n) pair reaches"""
    spb = ST_GROUPS // num_lods
    grid = min(-(-n // spb), GRID_CAP)
    passes = [len(range(b * spb, n, grid * spb)) for b in range(grid)]
    return dict(spb=spb, grid=grid, idle_groups=ST_GROUPS - spb * num_lods, tail_pass=n % spb != 0,
                second_pass_all=min(passes) >= 2, second_pass_some=max(passes) >= 2 > min(passes), max_passes=max(passes))


# ---------------------------------------------------------------------------------------------------- the float64 step
def _mm(a, b):
    """a [m, k] @ b [k, n]; forms every product (0 * inf = NaN, no zero skipped) when a non-finite value is present"""
    if bool(torch.isfinite(a).all()) and bool(torch.isfinite(b).all()):
        return a @ b
    return (a[:, :, None] * b[None, :, :]).sum(1)


def level_parts(case):
    """per level (weights f64 [n, 8], rows int64 [n, 8], valid bool [n]) from spc_exact_ref.weights and the tree's trinkets"""
    out = []
    for li in range(len(case["levels"])):
        w, valid = S.weights(case, li)
        p = case["chain"][:, li].numpy()
        rows = case["tree"].trinkets[np.where(valid, p, 0)].astype(np.int64)
        out.append((torch.from_numpy(w), torch.from_numpy(rows), torch.from_numpy(valid)))
    return out


def features(case, parts=None):
    """float64 [n, 16] = sum over levels of the trilinear blends, and the blends themselves"""
    parts = parts or level_parts(case)
    blends = []
    for (w, rows, valid), t in zip(parts, case["tables"]):
        t = t.half().double() if case["half_round"] else t.double()
        bl = (w[:, :, None] * t[rows]).sum(1) * valid[:, None]
        blends.append(bl.half().double() if case["half_round"] else bl)
    return sum(blends), blends


def inv_n_of(n):
    return float(np.float32(1.0) / np.float32(n))


def _sigmoid32(y):
    """1 / (1 + expf(-y)) in fp32, as the kernel's statement"""
    with np.errstate(over="ignore"):
        e = np.exp(-y.numpy().astype(np.float32))
        return torch.from_numpy((np.float32(1.0) / (np.float32(1.0) + e)).astype(np.float64))


def decoder_parts(case, gts=None, rgb_gts=None):
    """the float64 forward and decoder backward; one-output cases carry w2 [1, H], b2 [1] and one column in y, g, diff"""
    n, tex, fo = case["n"], case["tex"], 3 if case["pos_input"] else 0
    gts = case["gts"] if gts is None else gts
    parts = level_parts(case)
    feat, blends = features(case, parts)
    x = torch.cat([case["coords"].double(), feat], 1) if fo else feat
    w1, b1, w2, b2 = (case[k].double() for k in ("w1", "b1", "w2", "b2"))
    a = x @ w1.T + b1
    h = torch.relu(a)
    y = h @ w2.T + b2                                                     # [n, 1 or 4]
    inv_n = inv_n_of(n)
    d_sdf = y[:, -1] - gts.double().reshape(-1)
    if tex:
        rgb_gts = case["rgb_gts"] if rgb_gts is None else rgb_gts
        rgb = _sigmoid32(y[:, :3])
        d_rgb = rgb - rgb_gts.double()
        diff = torch.cat([d_rgb, d_sdf[:, None]], 1)
        g = torch.cat([2.0 * d_rgb * (rgb * (1.0 - rgb)) * inv_n, (2.0 * d_sdf * inv_n)[:, None]], 1)
    else:
        diff = d_sdf[:, None]
        g = 2.0 * diff * inv_n
    g_raw, g = g, g.float().double()                                      # rounded once
    gh = (g[:, :, None] * w2[None, :, :])                                  # [n, O, H] the terms of ga
    ga = torch.where(a > 0, gh.sum(1), torch.zeros_like(a))
    return dict(parts=parts, blends=blends, x=x, a=a, h=h, y=y, diff=diff, g=g, gh=gh, ga=ga, g_raw=g_raw, dfeat=_mm(ga, w1[:, fo:]), fo=fo, inv_n=inv_n)


def loss_of(case, p):
    sq = p["diff"] ** 2
    if not case["tex"]:
        return sq.sum().reshape(1) * p["inv_n"]
    dist, col = sq[:, 3].sum(), sq[:, :3].sum()
    return torch.stack([(dist + col) * p["inv_n"], dist, col])


def step_reference(case, gts=None, rgb_gts=None):
    """float64: dict(loss [1] or [3], pred [n], tables [L x [rows, 16]], w1, b1, w2, b2) - the gradients under their parameter's name"""
    p = decoder_parts(case, gts, rgb_gts)
    tables = []
    for (w, rows, valid), t in zip(p["parts"], case["tables"]):
        contrib = (w[:, :, None] * p["dfeat"][:, None, :])[valid]
        tables.append(torch.zeros(t.shape, dtype=F64).index_add_(0, rows[valid].reshape(-1), contrib.reshape(-1, C)))
    return dict(loss=loss_of(case, p), pred=p["y"][:, -1], tables=tables, w1=_mm(p["ga"].T, p["x"]), b1=p["ga"].sum(0),
                w2=_mm(p["g"].T, p["h"]).reshape(case["w2"].shape), b2=p["g"].sum(0))


def autograd_reference(case, dtype=F64):
    """the same numbers from torch autograd through oracle.octree_grid.octree_grid_interpolate and the oracle's decoder in `dtype`"""
    from oracle import nerf as onerf, octree_grid as og
    tr, tex, H = case["tree"], case["tex"], case["w1"].shape[0]
    levels = case["levels"]
    feats = [t.to(dtype).clone().requires_grad_(True) for t in case["tables"]]
    dec = onerf.OracleDecoder(case["w1"].shape[1], 4 if tex else 1, H, 1, True).to(dtype)
    with torch.no_grad():
        dec.layers[0].weight.copy_(case["w1"]); dec.layers[0].bias.copy_(case["b1"])
        dec.lout.weight.copy_(case["w2"].reshape(-1, H)); dec.lout.bias.copy_(case["b2"])
    # (octree_grid_interpolate walks lod 0 .. lod_idx of ONE list of active levels: the case's own list, which may start anywhere
    #  and have gaps)
    f = og.octree_grid_interpolate(tr.oracle_blas(), tr.trinkets, feats, case["coords"], len(levels) - 1, 0, list(levels), 'sum', C,
                                   case["half_round"]).to(dtype)
    x = torch.cat([case["coords"].to(dtype), f], 1) if case["pos_input"] else f
    y = dec(x)
    n = case["n"]
    l2 = ((y[:, -1] - case["gts"].to(dtype).reshape(-1)) ** 2).sum()
    if tex:
        rgb = ((torch.sigmoid(y[:, :3]) - case["rgb_gts"].to(dtype)) ** 2).sum()
        loss = (l2 + rgb) / n
        losses = torch.stack([loss, l2, rgb]).detach()
    else:
        loss = l2 / n
        losses = loss.detach().reshape(1)
    loss.backward()
    zero = lambda t: torch.zeros_like(t) if t.grad is None else t.grad
    return dict(loss=losses, pred=y[:, -1].detach(), tables=[zero(t) for t in feats], w1=dec.layers[0].weight.grad,
                b1=dec.layers[0].bias.grad, w2=dec.lout.weight.grad.reshape(case["w2"].shape), b2=dec.lout.bias.grad)


# ---------------------------------------------------------------------------------------------------- decoder patterns
def n_patterns(hidden, tex):
    """patterns after which every hidden unit has carried a non-zero output weight twice, under two different W1 (one chance sum
    of exactly zero does not leave an element dead)"""
    return 2 * max(1, -(-hidden // 16))


def make_decoder(hidden, tex, pos_input, pattern, modes, level_consts, seed):
    """W1 [H, in]: three entries of -1 / 1 per row; w2 / W2: -1 / 1 on the 16 units (16 pattern + j) mod H of each row (the distance
    row; a colour row shifted by 16 (o + 1)), 0 elsewhere; small integer biases.  Unit EDGE_UNIT reads +channel 0 - channel 1 +
    channel 15 with b1 = -(the constant channel 15 holds on the levels above the finest): channel 1 is a copy of channel 0, so its
    pre-activation is the finest level's blend of channel 15 - exactly 0 for part of the samples.  Colour mode 'half': units 2 and 3
    share row and bias and carry +1 / -1 in the colour row, b2 = 0; 'low' / 'high': b2 = -128 / +128, two non-zero entries."""
    rng = np.random.default_rng(seed + 31 * pattern)
    fo = 3 if pos_input else 0
    in_dim = fo + C
    w1 = np.zeros((hidden, in_dim), dtype=np.float32)
    for h in range(hidden):
        cols = (rng.choice(in_dim, size=3, replace=False) + pattern) % in_dim
        w1[h, cols] = rng.choice([-1.0, 1.0], size=3)
    b1 = rng.integers(-1, 2, size=hidden).astype(np.float32)
    w1[EDGE_UNIT] = 0.0
    w1[EDGE_UNIT, [fo, fo + 1, fo + C - 1]] = (1.0, -1.0, 1.0)
    b1[EDGE_UNIT] = -float(level_consts)
    rows = 4 if tex else 1
    w2 = np.zeros((rows, hidden), dtype=np.float32)
    live = (16 * pattern + np.arange(min(16, hidden))) % hidden
    w2[rows - 1, live] = rng.choice([-1.0, 1.0], size=live.shape[0])
    if pattern == 0:
        w2[rows - 1, EDGE_UNIT] = 1.0                                      # the edge unit's gradient would show: its output weight is live
    b2 = np.zeros(rows, dtype=np.float32)
    b2[rows - 1] = float(rng.integers(-2, 3))
    if tex:
        for o, mode in enumerate(modes):
            if mode == "half":
                assert hidden >= 4, "the 'half' colour mode needs a pair of hidden units"
                w1[3], b1[3] = w1[2], b1[2]
                w2[o, 2], w2[o, 3] = 1.0, -1.0
            else:
                units = (16 * (pattern + o + 1) + np.arange(min(2, hidden))) % hidden
                w2[o, units] = rng.choice([-1.0, 1.0], size=units.shape[0])
                b2[o] = -SAT_BIAS if mode == "low" else SAT_BIAS
    return tuple(torch.from_numpy(v) for v in (w1, b1, w2, b2))


# ---------------------------------------------------------------------------------------------------- exact inputs
def make_tables(tr, levels, half_round, seed):
    """integers in [-1, 1]; channel 1 copies channel 0; channel 15 is one constant per level above the finest; half_round: every third
    non-zero entry + 2^-13 (an fp32 value that the fp16 rounding turns back into the integer).  Returns (tables, sum of the constants)."""
    rng = np.random.default_rng(seed)
    tables, consts = [], 0
    for li, l in enumerate(levels):
        t = rng.integers(-1, 2, size=(tr.rows(l), C)).astype(np.float64)
        t[:, 1] = t[:, 0]
        if li < len(levels) - 1:
            c = (1, -1, 0)[li % 3]
            t[:, C - 1] = c
            consts += c
        if half_round:
            bump = (np.arange(t.size).reshape(t.shape) % 3 == 0) & (t != 0)     # (fp16 keeps 0 + 2^-13: zeros stay as they are)
            t = t + bump * 2.0 ** -13
            t[:, 1] = t[:, 0]
        t32 = t.astype(np.float32)
        assert np.array_equal(t32.astype(np.float64), t)
        tables.append(torch.from_numpy(t32))
    return tables, consts


def sample_cells(tr, levels, n, align, seed, all_miss=False):
    """cells [n, 3] of levels[-1] for make_case: occupied cells whose coordinates are multiples of 2^align; every 7th sample lies
    outside the unit cube (and so outside every cell), every 11th in an EMPTY cell of that lattice - it misses the finest level and
    whatever coarser levels its ancestors are missing from, and hits the others; all_miss: only samples outside the cube and samples
    in cells that are empty at every listed level"""
    rng = np.random.default_rng(seed)
    Lf = levels[-1]
    pts = tr.level_points(Lf)
    occ = pts[(pts % 2 ** align == 0).all(1)]
    assert occ.shape[0] >= 4, "the tree has no cells on this lattice"
    a = np.arange(0, 2 ** Lf, 2 ** align)
    if a.shape[0] ** 3 <= 2 ** 15:
        lat = np.stack(np.meshgrid(a, a, a, indexing='ij'), -1).reshape(-1, 3)
    else:
        lat = rng.integers(0, a.shape[0], size=(2 ** 15, 3)) * 2 ** align
    empty = lat[tr.lookup(Lf, lat) < 0]
    if all_miss:
        gone = empty[tr.lookup(levels[0], empty >> (Lf - levels[0])) < 0]
        assert gone.shape[0] >= 2, "no cell is empty at every listed level"
        cells = gone[rng.integers(0, gone.shape[0], size=n)]
        cells[::2] = S.OUTSIDE
        return cells
    cells = occ[rng.integers(0, occ.shape[0], size=n)]
    if n >= 8:
        cells[np.arange(n) % 7 == 6] = S.OUTSIDE
        if empty.shape[0]:
            partial = empty[tr.lookup(levels[0], empty >> (Lf - levels[0])) >= 0] if len(levels) > 1 else empty
            pick = partial if partial.shape[0] else empty
            m = np.arange(n) % 11 == 5
            cells[m] = pick[rng.integers(0, pick.shape[0], size=int(m.sum()))]
    return cells


def quantum(*tensors):
    """the largest power of two that divides every given value (1.0 when all are zero)"""
    best = None
    for t in tensors:
        v = np.asarray(t.double().reshape(-1).numpy() if isinstance(t, torch.Tensor) else t, dtype=np.float64).reshape(-1)
        v = v[(v != 0) & np.isfinite(v)]
        if v.size == 0:
            continue
        m, e = np.frexp(np.abs(v))
        M = (m * 2.0 ** 53).astype(np.uint64)
        tz = np.zeros(M.shape, dtype=np.int64)
        for sh in (32, 16, 8, 4, 2, 1):
            z = (M & np.uint64((1 << sh) - 1)) == 0
            tz += z * sh
            M = np.where(z, M >> np.uint64(sh), M)
        low = int((e.astype(np.int64) - 53 + tz).min())
        best = low if best is None else min(best, low)
    return 1.0 if best is None else 2.0 ** best


def _budget(name, abs_sum, terms, spans, extra=0.0):
    """one quantum for `terms` (and the pre-filled value); the absolute values (plus `extra`) sum to fewer than 2^24 quanta"""
    q = quantum(terms, *([torch.tensor([0.5])] if extra else []))
    top = (float(abs_sum.max()) if abs_sum.numel() else 0.0) + extra
    bits = float(np.log2(max(top / q, 1.0)))
    assert bits < 24.0, f"inputs are not exact: {name}: the partial sums leave fp32 ({bits:.1f} bits of quantum {q})"
    spans[name] = bits
    return q


def sg_fixed_point_exponent(n, absmax):
    """spc_grad.hip sg_scale (lines 52-63) with sg_clog (lines 539-543): the accumulators count multiples of 2^-sh,
    sh = 60 - clog - E, clog = ceil(log2(8 n)), E = the unbiased exponent of the batch's largest |weight * d features| (at least -126)"""
    clog = 3
    while (1 << (clog - 3)) < n:
        clog += 1
    E = max(int(np.floor(np.log2(absmax))), -126) if absmax > 0 else -126
    return 60 - clog - E


def check_exact_step(case, prefill=PREFILL_MAX):
    """assert the exactness conditions of the whole step; returns dict(spans {stage: bits used}, edge, zero shares, ...)"""
    n, tex = case["n"], case["tex"]
    assert n >= 1 and n & (n - 1) == 0, "n must be a power of two: 1 / n is exact"
    assert bool(torch.equal(case["gts"].float().double(), case["gts"].double())), "a target is no fp32 value"
    for k in ("w1", "w2"):
        assert bool(torch.equal(case[k].abs(), case[k].abs() ** 2)), f"{k} holds something else than -1 / 0 / 1"
    assert int((case["w1"] != 0).sum(1).max()) == 3 == int((case["w1"] != 0).sum(1).min()) and int((case["w2"] != 0).sum(1).max()) <= 16
    p = decoder_parts(case)
    fo = p["fo"]
    w1, b1, w2, b2 = (case[k].double() for k in ("w1", "b1", "w2", "b2"))
    spans = {}
    for li, ((w, rows, valid), t) in enumerate(zip(p["parts"], case["tables"])):
        t64 = t.half().double() if case["half_round"] else t.double()
        terms = (w[:, :, None] * t64[rows]) * valid[:, None, None]
        _budget(f"blend{li}", terms.abs().sum(1), terms, spans)
        if case["half_round"]:
            raw = terms.sum(1)
            assert bool(torch.equal(raw.half().double(), raw)), f"level {case['levels'][li]}: a blend is no fp16 value"
    if case["half_round"]:
        assert any(not bool(torch.equal(t.half().double(), t.double())) for t in case["tables"]), "the fp16 rounding of the tables changes nothing"
    _budget("features", sum(b.abs() for b in p["blends"]), torch.stack(p["blends"]), spans)
    x = p["x"]
    _budget("a", x.abs() @ w1.abs().T + b1.abs(), torch.cat([x.reshape(-1), b1]), spans)
    s2 = p["h"] @ w2.abs().T + b2.abs()                                    # [n, O]
    live_rows = [o for o in range(w2.shape[0]) if abs(float(b2[o])) != SAT_BIAS]
    _budget("y", s2[:, live_rows] + case["gts"].double().abs().reshape(-1, 1), torch.cat([p["h"].reshape(-1), b2[live_rows], case["gts"].double().reshape(-1)]), spans)
    if tex:
        y32 = p["y"][:, :3].float().numpy()
        with np.errstate(over="ignore"):
            e = np.exp(-y32)
        for o, mode in enumerate(case["modes"]):
            want = dict(half=1.0, low=np.inf, high=0.0)[mode]
            assert bool((e[:, o] == want).all()), f"colour {o} ({mode}): expf is not exactly {want}"
            if mode != "half":                                            # ... and stays so whatever the order of the row's sum
                assert float((p["h"] @ w2.abs().T)[:, o].max()) <= SAT_BIAS - 108.0, f"colour {o}: the row's sum can leave saturation"
        assert bool(torch.equal(case["rgb_gts"].float().double(), case["rgb_gts"].double()))
    sq = p["diff"] ** 2
    _budget("loss", sq.sum().reshape(1), sq, spans)
    assert bool(torch.equal(p["g"], p["g_raw"])), "inputs are not exact: g rounds"
    _budget("ga", p["gh"].abs().sum(1), p["gh"], spans)
    _budget("b2", p["g"].abs().sum(0), p["g"], spans, prefill)
    _budget("b1", p["ga"].abs().sum(0), p["ga"], spans, prefill)
    gr = p["g"][:, :, None] * p["h"][:, None, :]                           # [n, O, H]
    _budget("w2", gr.abs().sum(0), gr, spans, prefill)
    _budget("w1", p["ga"].abs().T @ x.abs(), torch.cat([(p["ga"][:, :, None] * x[:, None, :]).reshape(-1)]), spans, prefill)
    _budget("dfeat", p["ga"].abs() @ w1.abs()[:, fo:], p["ga"][:, :, None] * w1[None, :, fo:], spans)
    absmax, touched_zero, touched, quanta = 0.0, 0, 0, []
    for li, ((w, rows, valid), t) in enumerate(zip(p["parts"], case["tables"])):
        contrib = (w[:, :, None] * p["dfeat"][:, None, :])[valid]          # [nv, 8, C]
        assert bool(torch.equal(contrib.float().double(), contrib)), "a product weight * d features is no fp32 value"
        asum = torch.zeros(t.shape, dtype=F64).index_add_(0, rows[valid].reshape(-1), contrib.abs().reshape(-1, C))
        q = _budget(f"table{li}", asum, contrib, spans, prefill)
        if valid.any():
            absmax = max(absmax, float((w[valid].max(1).values * p["dfeat"][valid].abs().max(1).values).max()))
        total = torch.zeros(t.shape, dtype=F64).index_add_(0, rows[valid].reshape(-1), contrib.reshape(-1, C))
        wsum = torch.zeros(t.shape[0], dtype=F64).index_add_(0, rows[valid].reshape(-1), w[valid].reshape(-1))
        got_weight = (wsum > 0)[:, None] & (asum > 0)
        touched += int(got_weight.sum()); touched_zero += int((got_weight & (total == 0)).sum())
        quanta.append(q)
    if absmax > 0:                                                         # the accumulators' binary point lies below every term's
        sh = sg_fixed_point_exponent(n, absmax)
        assert 2.0 ** -(sh - 1) <= min(quanta), "a table term is no multiple of the fixed-point quantum"
    a = p["a"]
    edge = int(((a == 0) & (p["gh"].abs().sum(1) != 0)).sum())
    dec_live = dec_zero = 0
    for terms_abs, total in ((p["ga"].abs().T @ x.abs(), p["ga"].T @ x), (p["ga"].abs().sum(0), p["ga"].sum(0)),
                             (gr.abs().sum(0), gr.sum(0)), (p["g"].abs().sum(0), p["g"].sum(0))):
        dec_live += int((terms_abs > 0).sum()); dec_zero += int(((terms_abs > 0) & (total == 0)).sum())
    nonzero_diff = int((p["diff"][:, -1] != 0).sum())
    return dict(spans=spans, edge=edge, table_touched=touched, table_zero=touched_zero, dec_live=dec_live, dec_zero=dec_zero,
                nonzero_diff=nonzero_diff, relu_both=bool((a > 0).any()) and bool((a < 0).any()))


LADDER = ((1, 0), (0, 0), (0, 1), (0, 2), (0, 3), (0, 4), (0, 5), (0, 6), (0, 7), (0, 8))      # (b, align), richest first


def build_case(tree_name, levels, n, hidden, tex=False, pos_input=1, half_round=False, modes=("half", "half", "half"), pattern=0,
               b=1, align=0, seed=0, all_miss=False, inert_colour=False):
    """one case at a given (b, align); raises AssertionError where the inputs are not exact"""
    tr = tree(tree_name)
    levels = tuple(int(l) for l in levels)
    cells = sample_cells(tr, levels, n, align, seed + 7 * n + len(levels), all_miss)
    base = S.make_case(tr, cells, levels, C, True, b=b, seed=seed + n)
    tables, consts = make_tables(tr, levels, half_round, seed + 5)
    assert all(m in COLOUR_MODES for m in modes)
    if tex and hidden < 4:                                               # (no pair of units to spare: the colours saturate)
        modes = tuple("low" if m == "half" else m for m in modes)
    w1, b1, w2, b2 = make_decoder(hidden, tex, pos_input, pattern, modes, consts, seed + 17 * hidden)
    if inert_colour:                                                      # W2[0:3] = 0, b2[0:3] = 0, colour target 1/2: g_0..2 = 0 exactly
        w2[:3] = 0.0; b2[:3] = 0.0
    case = dict(base, tree_name=tree_name, tables=tables, half_round=bool(half_round), tex=bool(tex), pos_input=int(pos_input), n=n,
                w1=w1, b1=b1, w2=w2, b2=b2, modes=tuple(modes), pattern=pattern, align=align, hidden=hidden)
    case["gts"] = torch.zeros(n)
    case["rgb_gts"] = torch.full((n, 3), 0.5)
    p = decoder_parts(case)
    rng = np.random.default_rng(seed + 3 * n + 1)
    delta = rng.integers(-4, 5, size=n).astype(np.float64) / 4.0
    delta[0] = 0.75                                                       # (a single sample still has a gradient)
    edge = ((p["a"][:, EDGE_UNIT] == 0) & (case["w2"][-1, EDGE_UNIT] != 0)).numpy()
    delta[edge & (delta == 0)] = -0.5                                     # a sample on the relu edge has a gradient to lose
    gts = p["y"][:, -1] + torch.from_numpy(delta)
    assert bool(torch.equal(gts.float().double(), gts)), "inputs are not exact: a target is no fp32 value"
    case["gts"] = gts.float()
    if tex and not inert_colour:
        col = np.zeros((n, 3))
        for o, mode in enumerate(modes):
            if mode == "half":
                col[:, o] = 0.5 + rng.choice([-1.0, 1.0], size=n) * 2.0 ** -rng.integers(1, 4, size=n)
            elif mode == "low":
                col[:, o] = rng.integers(1, 5, size=n) / 4.0              # rgb = 0: a non-zero difference
            else:
                col[:, o] = rng.integers(0, 4, size=n) / 4.0              # rgb = 1
        case["rgb_gts"] = torch.from_numpy(col.astype(np.float32))
    case["report"] = check_exact_step(case)
    case["want"] = step_reference(case)
    return case


_cases = {}


def exact_case(tree_name, levels, n, hidden, **kw):
    """the first rung of LADDER (offsets k / 2, then cell origins on coarser and coarser lattices) that check_exact_step accepts, with
    the conditions on what the case must reach asserted; cached"""
    key = (tree_name, tuple(levels), n, hidden, tuple(sorted(kw.items())))
    if key in _cases:
        return _cases[key]
    last = None
    for b, align in LADDER:
        if align > levels[-1]:
            continue
        try:
            case = build_case(tree_name, levels, n, hidden, b=b, align=align, **kw)
        except AssertionError as e:
            last = e
            continue
        rep = case["report"]
        if not kw.get("all_miss"):
            assert 2 * rep["nonzero_diff"] >= n, "fewer than half of the samples have a non-zero difference"
            if n >= 16:
                assert rep["edge"] >= 1, "no sample sits on the relu edge with a gradient to lose"
            assert rep["table_zero"] <= ZERO_CAP * max(rep["table_touched"], 1), ("tables hide in zeros", rep)
            assert rep["dec_zero"] <= ZERO_CAP * max(rep["dec_live"], 1), ("decoder gradients hide in zeros", rep)
        _cases[key] = case
        return case
    raise AssertionError(f"no exact case for {key}: {last}")


# ---------------------------------------------------------------------------------------------------- derived bounds (family B)
U = 2.0 ** -24


def inexact_case(case, n):
    """the first n samples (n no power of two) of an exact case: the forward, diff and g (rounded once) are still reproduced exactly by
    the reference - inv_n = fl(1 / n) is no power of two, so only the sums of the gradients round"""
    out = dict(case)
    for k in ("coords", "chain", "gts", "rgb_gts"):
        out[k] = case[k][:n].contiguous()
    out["n"] = out["N"] = n
    out.pop("report", None)
    out["want"] = step_reference(out)
    return out


def derived_bounds(case, before):
    """per output element: (k + 2) 2^-24 A, k = the number of non-zero terms of the element, A = the float64 sum of their absolute
    values plus the absolute pre-filled value (any summation tree of k terms, each product rounded once, added to the pre-filled
    value: every term passes through at most k + 1 roundings; (k + 1)(k + 2) 2^-24 <= 1 for k <= 4000 keeps the second order inside).
    Tables add the propagated bound of every contributing sample's d features times its weight, and one fixed-point quantum per
    contribution (twice 2^-sh: the kernel takes E from ITS largest product, whose exponent can differ by one from the reference's)."""
    p = decoder_parts(case)
    n, fo = case["n"], p["fo"]
    x, ga, g, h, gh = p["x"], p["ga"], p["g"], p["h"], p["gh"]
    w1 = case["w1"].double()
    live = (p["a"] > 0).double()
    gh_live = gh * live[:, None, :]                                        # the leaf terms of ga: [n, O, H]
    k_ga, a_ga = (gh_live != 0).double().sum(1), gh_live.abs().sum(1)      # [n, H]
    nz = lambda t: (t != 0).double()
    out = {}
    k = k_ga.T @ nz(x); A = a_ga.T @ x.abs()
    out["w1"] = (k + 2) * U * (A + before["w1"].double().abs())
    out["b1"] = (k_ga.sum(0) + 2) * U * (a_ga.sum(0) + before["b1"].double().abs())
    k = torch.einsum("no,nh->oh", nz(g), nz(h)); A = torch.einsum("no,nh->oh", g.abs(), h)
    out["w2"] = ((k + 2) * U * (A + before["w2"].double().reshape(k.shape).abs())).reshape(case["w2"].shape)
    out["b2"] = (nz(g).sum(0) + 2) * U * (g.abs().sum(0) + before["b2"].double().abs())
    out["loss"] = (n + 2) * U * (loss_of(case, dict(p, diff=p["diff"].abs())))
    k_df = k_ga @ nz(w1[:, fo:]); a_df = a_ga @ w1[:, fo:].abs()
    e_df = (k_df + 1) * U * a_df                                           # [n, C] error of the kernel's d features
    absmax = 0.0
    for (w, rows, valid) in p["parts"]:
        if valid.any():
            absmax = max(absmax, float((w[valid].max(1).values * p["dfeat"][valid].abs().max(1).values).max()))
    quantum_fp = 2.0 * 2.0 ** -sg_fixed_point_exponent(n, absmax) if absmax > 0 else 0.0
    out["tables"] = []
    for (w, rows, valid), t, bf in zip(p["parts"], case["tables"], before["tables"]):
        r = rows[valid].reshape(-1)
        add = lambda v: torch.zeros(t.shape, dtype=F64).index_add_(0, r, v.reshape(-1, C))
        contrib = (w[:, :, None] * p["dfeat"][:, None, :])[valid]
        k = add(nz(contrib)); A = add(contrib.abs())
        prop = add((w[:, :, None] * e_df[:, None, :])[valid])
        out["tables"].append((k + 2) * U * (A + bf.double().abs()) + prop * (1 + (k + 2) * U) + k * quantum_fp)
    return out


# ---------------------------------------------------------------------------------------------------- the cases of the GPU file
# (tree, levels): 1, 2, 3, 4, 5, 6, 8 and 9 levels (16, 8, 5, 4, 3, 2, 2 and 1 samples per pass), lists that start above level 1 and
# lists with gaps
LEVEL_LISTS = (("small", (5,)), ("small", (4, 5)), ("small", (3, 4, 5)), ("small", (2, 3, 4, 5)), ("small", (1, 2, 3, 4, 5)),
               ("small", (0, 1, 2, 3, 4, 5)), ("deep", (1, 2, 3, 4, 5, 6, 7, 8)), ("deep", (2, 3, 4, 5, 6, 7, 8, 9, 10)),
               ("small", (1, 3, 5)), ("deep", (2, 5, 9)))
NS = (1, 2, 16, 64, 512)
BIG = (("small", (0, 1, 2, 3, 4, 5), 4096), ("small", (3, 4, 5), 8192))      # every workgroup two passes; some two, some one
HIDDENS = (1, 16, 17, 24, 128, 256)
INEXACT_NS = (3, 37, 511, 513)
INEXACT_BIG = ("small", (0, 1, 2, 3, 4, 5), 2049)
