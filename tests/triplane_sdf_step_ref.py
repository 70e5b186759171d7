"""float64 restatement of the fused triplanar SDF training step (csrc/triplane_sdf_train.hip: forward, loss = sum((pred - gt)^2) / n
and every gradient), and a generator of exactly representable training cases.  Test infrastructure only; host only (numpy + torch
CPU), built on tests/triplane_sdf_eval_ref.py (source_index, features, reference, exact_points, exact_field).

The gradients are written out, not taken from autograd: with x = [position, features], a = W1 x + b1, h = relu(a), pred = w2 . h + b2,
g = 2 (pred - gt) / n:  d b2 = sum g,  d w2 = h^T g,  ga = g w2 [a > 0],  d b1 = sum ga,  d W1 = ga^T x,  d features = ga W1[:, 3:],
and the gradient of a plane is a float64 scatter-add of corner weight * d features over the (up to) four texels of the lookup - a
corner with x0 + 1 >= size or y0 + 1 >= size is left out, as in the forward; 'cat': a column belongs to one (level, plane, channel),
'sum': every level receives the gradient of the summed column.  The corner weights come from the fp32 source coordinate the kernel
forms (triplane_sdf_eval_ref.source_index); tx = ix - floor(ix) is exact in fp32.

Exact cases.  The points of triplane_sdf_eval_ref.exact_points and a field of exact_field (w2 with at most 16 non-zero entries): blend
factors, features and decoder inputs are multiples of q = 2^-bits.  The target of a sample is its own float64 prediction plus a
multiple of 1/4 in [-1, 1], so pred - gt is that small dyadic number and, n being a power of two, g = 2 (pred - gt) / n a multiple of
qg = 1 / (2 n).  check_exact_step then proves per case that every product and every partial sum of the loss, the decoder backward and
the plane scatter - including the value a gradient buffer was pre-filled with - is a multiple of one quantum with fewer than 2^24
quanta IN ANY ORDER OF ADDITION (it sums absolute values): a kernel must equal the float64 result BIT FOR BIT, atomics or not.  A
failure there blames the inputs, not the kernel.
"""
import numpy as np
import torch

import triplane_sdf_eval_ref as R

F64 = torch.float64
PREFILL_MAX = 2.0                      # |value| a gradient buffer may be pre-filled with (multiples of 1/2)
GT_BITS = 2                            # pred - gt is a multiple of 2^-GT_BITS in an exact case
DECODER = ("w1", "b1", "w2", "b2")


def lookup_corners(gx, gy, size):
    """the four corners 00, 01, 10, 11 of one lookup: (weights float64 [n, 4] - zero where the corner is left out -, texel offsets
    y * size + x int64 [n, 4] - clamped into the plane where left out -, kept bool [n, 4])"""
    ix, iy = R.source_index(gx, size), R.source_index(gy, size)
    fx, fy = np.floor(ix), np.floor(iy)
    x0, y0 = torch.from_numpy(fx.astype(np.int64)), torch.from_numpy(fy.astype(np.int64))
    tx, ty = torch.from_numpy(ix - fx).double(), torch.from_numpy(iy - fy).double()
    ws, offs, oks = [], [], []
    for dy, dx, w in ((0, 0, (1 - tx) * (1 - ty)), (0, 1, tx * (1 - ty)), (1, 0, (1 - tx) * ty), (1, 1, tx * ty)):
        ok = (x0 + dx < size) & (y0 + dy < size)
        ws.append(torch.where(ok, w, torch.zeros_like(w)))
        offs.append(torch.clamp(y0 + dy, max=size - 1) * size + torch.clamp(x0 + dx, max=size - 1))
        oks.append(ok)
    return torch.stack(ws, 1), torch.stack(offs, 1), torch.stack(oks, 1)


def plane_lookups(fld, coords):
    """per plane, in the field's plane order: (weights, offsets, kept, first feature-gradient column)"""
    c = coords.float().numpy()
    F, cat = R.plane_features(fld), fld["multiscale"] == 'cat'
    out = []
    for l in range(R.num_lods(fld)):
        size = int(fld["planes"][3 * l].shape[-1])
        for p, (gx, gy) in enumerate(((c[:, 1], c[:, 2]), (c[:, 0], c[:, 2]), (c[:, 0], c[:, 1]))):
            out.append(lookup_corners(gx, gy, size) + ((l * 3 * F if cat else 0) + p * F,))
    return out


def decoder_parts(fld, coords, gts):
    """the float64 forward and decoder backward: dict of x, a, h, pred, diff, g, ga, dfeat"""
    n = coords.shape[0]
    x = torch.cat([coords.double(), R.features(fld, coords)], dim=1)
    w1, b1, w2, b2 = (fld[k].double() for k in DECODER)
    a = x @ w1.T + b1
    h = torch.relu(a)
    pred = h @ w2 + b2                                   # [n]
    diff = pred - gts.double().reshape(-1)
    g = 2.0 * diff / n
    ga = g[:, None] * w2[None, :] * (a > 0)
    return dict(x=x, a=a, h=h, pred=pred, diff=diff, g=g, ga=ga, dfeat=ga @ w1[:, 3:])


def step_reference(fld, coords, gts):
    """float64: dict(loss [1], pred [n], planes (list, each [F, R, R]), w1, b1, w2, b2) - the gradients under their parameter's name"""
    p = decoder_parts(fld, coords, gts)
    n = coords.shape[0]
    F = R.plane_features(fld)
    planes = []
    for plane, (w, off, _, col) in zip(fld["planes"], plane_lookups(fld, coords)):
        size = int(plane.shape[-1])
        d = p["dfeat"][:, col:col + F]                   # [n, F]
        grad = torch.zeros(size * size, F, dtype=F64)
        grad.index_add_(0, off.reshape(-1), (w[:, :, None] * d[:, None, :]).reshape(-1, F))
        planes.append(grad.T.reshape(F, size, size).contiguous())
    return dict(loss=(p["diff"] ** 2).sum().reshape(1) / n, pred=p["pred"], planes=planes, w1=p["ga"].T @ p["x"], b1=p["ga"].sum(0),
                w2=p["h"].T @ p["g"], b2=p["g"].sum().reshape(1))


def autograd_reference(fld, coords, gts):
    """the same numbers from torch autograd in float64 through oracle/triplanar.py (torch's CPU grid_sample on float64 planes and
    the fp32 positions widened to float64).  Its source coordinate is formed in float64: it is the kernel's fp32 one only where that
    is exact - coordinates on a binary lattice over planes with power-of-two spans (lattice_points below)."""
    from oracle import triplanar as otri
    planes = [q.double().reshape(1, *q.shape[-3:]).clone().requires_grad_(True) for q in fld["planes"]]
    dec = {k: fld[k].double().clone().requires_grad_(True) for k in DECODER}
    L = R.num_lods(fld)
    c = coords.float().double()
    feats = otri.interpolate([tuple(planes[3 * l:3 * l + 3]) for l in range(L)], c, L - 1, fld["multiscale"])
    x = torch.cat([c, feats], dim=1)
    pred = torch.relu(x @ dec["w1"].T + dec["b1"]) @ dec["w2"] + dec["b2"]
    loss = ((pred - gts.double().reshape(-1)) ** 2).sum() / coords.shape[0]
    loss.backward()
    return dict(loss=loss.detach().reshape(1), pred=pred.detach().reshape(-1), planes=[q.grad[0] for q in planes],
                **{k: v.grad for k, v in dec.items()})


def lattice_points(n, seed=0, frac_bits=20):
    """generic positions whose fp32 source coordinate is exact on a plane with a power-of-two span: multiples of 2^-frac_bits in
    [-1.3, 1.3] (g + 1 < 2.3 keeps 2^-20 within fp32's 24 bits); a third outside the cube, some exactly on +-1, one at the origin"""
    rng = np.random.default_rng(seed)
    unit = 2 ** frac_bits
    m = rng.integers(-unit, unit + 1, size=(n, 3))
    out = np.arange(n) % 3 == 2
    pick = rng.integers(0, 3, size=n)
    sign = rng.choice([-1, 1], size=n)
    far = rng.integers(unit, int(1.3 * unit), size=n)
    m[out, pick[out]] = (sign * far)[out]
    face = np.arange(n) % 5 == 1
    m[face, pick[face]] = (sign * unit)[face]
    m[0] = 0
    g = (m.astype(np.float64) / unit).astype(np.float32)
    assert np.array_equal(g.astype(np.float64) * unit, m.astype(np.float64))
    return torch.from_numpy(g)


# ---------------------------------------------------------------------------------------------------- exact cases
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
    _budget("pred - gt", s2 + gts.double().reshape(-1).abs(), torch.cat([p["pred"], gts.double().reshape(-1)]), q, spans)
    qd = 2.0 ** -GT_BITS
    _budget("diff", p["diff"].abs(), p["diff"], qd, spans)
    sq = p["diff"] ** 2
    _budget("loss", sq.sum().reshape(1), sq, qd * qd, spans)
    qg = 2.0 * qd / n                                    # the quantum of g (2 / n is a power of two)
    _budget("b2", p["g"].abs().sum().reshape(1), p["g"], qg, spans, prefill)
    _budget("b1", p["ga"].abs().sum(0), p["ga"], qg, spans, prefill)
    gr = p["g"][:, None] * p["h"]
    _budget("w2", gr.abs().sum(0), gr, qg * q, spans, prefill)
    _budget("w1", p["ga"].abs().T @ p["x"].abs(), p["ga"][:, :, None] * p["x"][:, None, :], qg * q, spans, prefill)
    _budget("dfeat", p["ga"].abs() @ fld["w1"].double().abs()[:, 3:], p["dfeat"], qg, spans)
    F = R.plane_features(fld)
    top, terms = [], []
    for plane, (w, off, _, col) in zip(fld["planes"], plane_lookups(fld, coords)):
        size = int(plane.shape[-1])
        t = w[:, :, None] * p["dfeat"][:, None, col:col + F]
        acc = torch.zeros(size * size, F, dtype=F64)
        acc.index_add_(0, off.reshape(-1), t.abs().reshape(-1, F))
        top.append(acc.reshape(-1))
        terms.append(t.reshape(-1))
    _budget("planes", torch.cat(top), torch.cat(terms), qg * q, spans, prefill)
    return spans


def coverage(fld, coords):
    """what a batch exercises: dict(reflected, edge, on_texel, shared) - samples outside the cube, lookups with a corner left out,
    lookups with tx == ty == 0, texels that receive a non-zero weight from several samples"""
    c = coords.float().numpy()
    edge = on_texel = shared = 0
    for plane, (w, off, ok, _) in zip(fld["planes"], plane_lookups(fld, coords)):
        size = int(plane.shape[-1])
        if size > 1:
            edge += int((~ok).any(1).sum())
            on_texel += int(((w != 0).sum(1) == 1).sum())
        hit = torch.zeros(coords.shape[0], size * size)
        hit.scatter_(1, off, (w != 0).float())
        shared += int(((hit > 0).sum(0) >= 2).sum())
    return dict(reflected=int((np.abs(c) > 1).any(1).sum()), edge=edge, on_texel=on_texel, shared=shared)


def exact_step_case(hidden=128, F=4, multiscale='sum', sizes=R.EXACT_SIZES[-1:], n=512, seed=0, b=1, all_miss=False):
    """dict(field, coords, gts, bits, spans, want, coverage).  exact_points puts every 5th point on a texel line of every level,
    every 7th on g == 1 (the + 1 corners fall outside the plane), every 11th on g == -1, and ranges to |g| = 1.5 (reflected).
    all_miss: b1 = -64, every pre-activation negative.  Asserted for n >= 16: the relu is hit on both sides (all_miss: on neither),
    some plane has a non-zero gradient (their number is kept in coverage['planes_with_gradient']), and the coverage above."""
    fld = R.exact_field(hidden, F, multiscale, sizes, seed=seed + 17 * hidden + F, w2_nonzero=16)
    if all_miss:
        fld["b1"] = torch.full_like(fld["b1"], -64.0)
    coords = R.exact_points(n, b=b, seed=seed + n)
    rng = np.random.default_rng(seed + 3 * n + 1)
    bits = R._bits(b, sizes)
    pred = R.reference(fld, coords).reshape(-1)
    delta = torch.from_numpy(rng.integers(-4, 5, size=n).astype(np.float64) / 4.0)
    delta[0] = 0.75                                      # (a single sample still has a gradient)
    gts = (pred + delta).float()
    assert bool(torch.equal(gts.double(), pred + delta))
    spans = check_exact_step(fld, coords, gts, bits)
    want = step_reference(fld, coords, gts)
    p = decoder_parts(fld, coords, gts)
    cov = coverage(fld, coords)
    if all_miss:
        assert bool((p["a"] < 0).all()), "a pre-activation is not negative"
        assert all(bool((g == 0).all()) for g in want["planes"]) and bool((want["w1"] == 0).all()) and float(want["b2"]) != 0
    elif n >= 16:
        assert hidden == 1 or (bool((p["a"] > 0).any()) and bool((p["a"] <= 0).any())), "the relu is hit on one side only"
        cov["planes_with_gradient"] = sum(bool((g != 0).any()) for g in want["planes"])
        assert cov["planes_with_gradient"] >= 1, "no plane receives a gradient"
        assert cov["reflected"] >= 1 and cov["on_texel"] >= 1 and cov["shared"] >= 1, cov
        assert cov["edge"] >= 1 or all(int(q.shape[-1]) == 1 for q in fld["planes"]), cov
    return dict(field=fld, coords=coords, gts=gts, bits=bits, spans=spans, want=want, coverage=cov)
