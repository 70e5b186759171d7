"""float64 restatement of the fused hash-grid SDF training step (csrc/hash_sdf_train.hip: forward, loss = sum((pred - gt)^2) / n and
all five gradients), and a generator of exactly representable training cases.  Test infrastructure only; host only (numpy + torch
CPU), built on tests/hash_sdf_eval_ref.py (level_blends, features, reference) and oracle/hashgrid.py.

The gradients are written out, not taken from autograd: with x = [position, features], a = W1 x + b1, h = relu(a), pred = w2 . h + b2,
g = 2 (pred - gt) / n:  d b2 = sum g,  d w2 = h^T g,  ga = g w2 [a > 0],  d b1 = sum ga,  d W1 = ga^T x,  d features = ga W1[:, 3:],
and the table gradient is a float64 scatter-add of blend factor * d features over the eight corner rows of every live level ('cat':
the levels below lod_idx, each with its own columns; 'sum': every level, each with the whole feature gradient).

Exact cases.  The points of hash_sdf_eval_ref.exact_points at b = 0 on the sub-grid of every `step`-th finest cell: blend factors,
level blends and decoder inputs are multiples of q = 2^-bits (bits = 6 at step 2, 4 at step 4).  Tables hold integers in [-1, 1], W1
three entries of -1 / 1 per row, w2 -1 / 0 / 1 with at most 16 non-zero entries, the biases small integers - and the target of a
sample is its own float64 prediction plus a multiple of 1/4 in [-1, 1], so pred - gt is that small dyadic number and, n being a
power of two, g = 2 (pred - gt) / n a multiple of 2 q / n.  check_exact_step then proves per case that every product and every
partial sum of the loss, the decoder backward and the table scatter - including the value a gradient buffer was pre-filled with - is
a multiple of one quantum with fewer than 2^24 quanta IN ANY ORDER OF ADDITION (it sums absolute values): a kernel must equal the
float64 result BIT FOR BIT, float atomics or not.  A failure there blames the inputs, not the kernel.
"""
import numpy as np
import torch

import hash_sdf_eval_ref as R
from oracle import hashgrid as ohg

F64 = torch.float64
PREFILL_MAX = 2.0                      # |value| a gradient buffer may be pre-filled with (multiples of 1/2)


def level_corners(fld, coords):
    """per level (blend factors float64 [n, 8], table rows int64 [n, 8]) - the factors from the fp32 position the kernel forms, as
    hash_sdf_eval_ref.level_blends takes them"""
    T = 2 ** fld["bitwidth"]
    c32 = coords.float()
    out = []
    for l, res in enumerate(fld["resolutions"]):
        _, idx = ohg.corner_setup(c32, int(res), T)
        x = ((c32.double() * 0.5 + 0.5) * float(res)).float()
        x = torch.clamp(x, min=0.0, max=float(np.float32(res - 1 - 1e-5)))
        f = (x - torch.floor(x)).double()
        g = 1.0 - f
        w = torch.stack([(f if j & 4 else g)[:, 0] * (f if j & 2 else g)[:, 1] * (f if j & 1 else g)[:, 2] for j in range(8)], 1)
        out.append((w, int(fld["begin"][l]) + idx))
    return out


def live_levels(fld):
    """[(level, first feature-gradient column)] of the levels that are gathered - and therefore receive a gradient"""
    L, F = len(fld["resolutions"]), fld["table"].shape[1]
    if fld["multiscale"] == 'cat':
        return [(l, l * F) for l in range(min(fld["lod_idx"], L))]
    return [(l, 0) for l in range(L)]


def decoder_parts(fld, coords, gts):
    """the float64 forward and decoder backward: dict of x, a, h, pred, diff, g, ga, dfeat"""
    n = coords.shape[0]
    x = torch.cat([coords.double(), R.features(fld, coords)], dim=1)
    w1, b1, w2, b2 = (fld[k].double() for k in ("w1", "b1", "w2", "b2"))
    a = x @ w1.T + b1
    h = torch.relu(a)
    pred = h @ w2 + b2                                   # [n]
    diff = pred - gts.double().reshape(-1)
    g = 2.0 * diff / n
    ga = g[:, None] * w2[None, :] * (a > 0)
    return dict(x=x, a=a, h=h, pred=pred, diff=diff, g=g, ga=ga, dfeat=ga @ w1[:, 3:])


def step_reference(fld, coords, gts):
    """float64: dict(loss [1], pred [n], table, w1, b1, w2, b2) - the five gradients under their parameter's name"""
    assert fld["table"].dtype == torch.float32, "the table is f32 under training"
    p = decoder_parts(fld, coords, gts)
    n = coords.shape[0]
    F = fld["table"].shape[1]
    table = torch.zeros(fld["table"].shape, dtype=F64)
    corners = level_corners(fld, coords)
    for l, col in live_levels(fld):
        w, rows = corners[l]
        d = p["dfeat"][:, col:col + F]
        table.index_add_(0, rows.reshape(-1), (w[:, :, None] * d[:, None, :]).reshape(-1, F))
    return dict(loss=(p["diff"] ** 2).sum().reshape(1) / n, pred=p["pred"], table=table, w1=p["ga"].T @ p["x"], b1=p["ga"].sum(0),
                w2=p["h"].T @ p["g"], b2=p["g"].sum().reshape(1))


def autograd_reference(fld, coords, gts):
    """the same six numbers from torch autograd through hash_sdf_eval_ref.reference in float64"""
    leaves = {k: fld[k].double().clone().requires_grad_(True) for k in ("table", "w1", "b1", "w2", "b2")}
    # (level_blends rounds through the table dtype unless that is f32: through float64 that is a differentiable no-op)
    pred = R.reference(dict(fld, **leaves), coords)
    loss = ((pred - gts.double().reshape(-1, 1)) ** 2).sum() / coords.shape[0]
    loss.backward()
    return dict(loss=loss.detach().reshape(1), pred=pred.detach().reshape(-1), **{k: v.grad for k, v in leaves.items()})


# ---------------------------------------------------------------------------------------------------- exact cases
def exact_step_field(hidden, F, multiscale, lod_idx, resolutions=R.EXACT_RES, bitwidth=R.EXACT_BITWIDTH, seed=0):
    """hash_sdf_eval_ref.exact_field for any list of power-of-two resolutions up to 32 and any table size, w2 with at most 16
    non-zero entries"""
    rng = np.random.default_rng(seed)
    _, begin = ohg.table_layout(resolutions, 2 ** bitwidth)
    table = torch.from_numpy(rng.integers(-1, 2, size=(int(begin[-1]), F)).astype(np.float32))
    K = len(resolutions) * F if multiscale == 'cat' else F
    w1 = np.zeros((hidden, 3 + K), dtype=np.float32)
    for h in range(hidden):
        cols = rng.choice(3 + K, size=3, replace=False)
        w1[h, cols] = rng.choice([-1.0, 1.0], size=3)
    b1 = rng.integers(-1, 2, size=hidden).astype(np.float32)
    w2 = rng.choice([-1.0, 1.0], size=hidden).astype(np.float32)
    if hidden > 16:
        w2[rng.permutation(hidden)[16:]] = 0.0
    b2 = rng.integers(-2, 3, size=1).astype(np.float32)
    return dict(table=table, begin=torch.from_numpy(begin), resolutions=[int(r) for r in resolutions], bitwidth=int(bitwidth),
                multiscale=multiscale, lod_idx=int(lod_idx), w1=torch.from_numpy(w1), b1=torch.from_numpy(b1),
                w2=torch.from_numpy(w2), b2=torch.from_numpy(b2))


def _budget(name, terms_abs_sum, values, quantum, spans, extra=0.0):
    """every value is a multiple of `quantum`; the sum of absolute values (plus `extra`) stays below 2^24 quanta"""
    v = values.double()
    assert bool(torch.equal(torch.round(v / quantum) * quantum, v)), f"{name}: a term is off the quantum grid"
    top = float(terms_abs_sum.max()) + extra if terms_abs_sum.numel() else extra
    bits = float(np.log2(max(top / quantum, 1.0)))
    assert bits < 24.0, f"{name}: the partial sums leave fp32 ({bits:.1f} bits)"
    spans[name] = bits
    return bits


def check_exact_step(fld, coords, gts, bits, prefill=PREFILL_MAX):
    """assert the exactness conditions of the whole step; returns {stage: bits used}.  The forward's are check_exact's."""
    n = coords.shape[0]
    assert n >= 1 and n & (n - 1) == 0, "n must be a power of two: 1 / n is exact"
    R.check_exact(fld, coords, bits)
    q = 2.0 ** -bits
    p = decoder_parts(fld, coords, gts)
    assert bool(torch.equal(gts.float().double(), gts.double())), "a target is no fp32 value"
    assert bool(torch.equal(torch.abs(fld["w1"]), torch.abs(fld["w1"]) ** 2)) and bool(torch.equal(fld["w2"].abs(), fld["w2"].abs() ** 2))
    spans = {}
    s2 = p["h"] @ fld["w2"].double().abs() + fld["b2"].double().abs()
    _budget("diff", s2 + gts.double().reshape(-1).abs(), p["diff"], q, spans)
    sq = p["diff"] ** 2
    _budget("loss", sq.sum().reshape(1), sq, q * q, spans)
    qg = 2.0 * q / n                                     # the quantum of g (2 / n is a power of two)
    _budget("b2", p["g"].abs().sum().reshape(1), p["g"], qg, spans, prefill)
    _budget("b1", p["ga"].abs().sum(0), p["ga"], qg, spans, prefill)
    gr = p["g"][:, None] * p["h"]
    _budget("w2", gr.abs().sum(0), gr, qg * q, spans, prefill)
    _budget("w1", p["ga"].abs().T @ p["x"].abs(), p["ga"][:, :, None] * p["x"][:, None, :], qg * q, spans, prefill)
    _budget("dfeat", p["ga"].abs() @ fld["w1"].double().abs()[:, 3:], p["dfeat"], qg, spans)
    F = fld["table"].shape[1]
    acc = torch.zeros(fld["table"].shape, dtype=F64)
    terms = []
    corners = level_corners(fld, coords)
    for l, col in live_levels(fld):
        w, rows = corners[l]
        t = w[:, :, None] * p["dfeat"][:, None, col:col + F]
        acc.index_add_(0, rows.reshape(-1), t.abs().reshape(-1, F))
        terms.append(t.reshape(-1))
    _budget("table", acc, torch.cat(terms) if terms else torch.zeros(0, dtype=F64), qg * q, spans, prefill)
    return spans


EXACT_STEP = {1: 2, 16: 2, 512: 4}                       # n -> every `step`-th finest cell


def exact_step_case(hidden=128, F=8, multiscale='cat', lod_idx=3, n=512, resolutions=R.EXACT_RES, bitwidth=8, seed=0):
    """dict(field, coords, gts, bits, spans, want).  Every 7th point lies outside the cube (a coordinate of -1.25 or -1.5: clamped
    to the first cell, position 0), every 5th on a cell face of every level; asserted: the relu is hit on both sides, every live level
    has non-zero table gradients, and several samples add to the same table row"""
    step = EXACT_STEP[n]
    fld = exact_step_field(hidden, F, multiscale, lod_idx, resolutions, bitwidth, seed=seed + 17 * hidden + F)
    coords = R.exact_points(n, b=0, step=step, seed=seed + n)
    rng = np.random.default_rng(seed + 3 * n + 1)
    out = torch.arange(n) % 7 == 6
    if n > 1:
        axis = torch.from_numpy(rng.integers(0, 3, size=n))
        coords[out, axis[out]] = torch.from_numpy(rng.choice([-1.25, -1.5], size=int(out.sum())).astype(np.float32))
    bits = R._bits(0, step)
    pred = R.reference(fld, coords).reshape(-1)
    delta = torch.from_numpy(rng.integers(-4, 5, size=n).astype(np.float64) / 4.0)
    delta[0] = 0.75                                      # (a single sample still has a gradient)
    gts = (pred + delta).float()
    assert bool(torch.equal(gts.double(), pred + delta))
    spans = check_exact_step(fld, coords, gts, bits)
    want = step_reference(fld, coords, gts)
    p = decoder_parts(fld, coords, gts)
    live = live_levels(fld)
    if n >= 16:
        assert bool((p["a"] > 0).any()) and bool((p["a"] <= 0).any()), "the relu is hit on one side only"
        begin = fld["begin"]
        for l, _ in live:
            assert bool((want["table"][int(begin[l]):int(begin[l + 1])] != 0).any()), f"level {l} receives no gradient"
        if live:
            touched = torch.zeros(fld["table"].shape[0])
            for l, _ in live:
                w, rows = level_corners(fld, coords)[l]
                hit = torch.zeros(n, fld["table"].shape[0])
                hit.scatter_(1, rows, (w != 0).float())
                touched += (hit > 0).float().sum(0)
            assert int((touched >= 2).sum()) >= 4, "no table row is shared by several samples"
    return dict(field=fld, coords=coords, gts=gts, bits=bits, spans=spans, want=want)
