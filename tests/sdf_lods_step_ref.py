"""float64 restatement of the fused all-LOD octree SDF training step (csrc/spc_grad.hip: wisp_sdf_lods_train_step =
sdf_lods_train_kernel + sdf_lods_train_reduce_kernel + the wide scatter + finalize), a generator of exactly representable cases and the
checker that proves them exact.  Test infrastructure only; host only.  Everything about one LOD - the tree, the trilinear weights, the
decoder patterns, the exact tables and targets - is tests/sdf_step_exact_ref.py's (X) and tests/spc_exact_ref.py's (S), imported and
left as they are.

With L levels, k = 0..L-1, the step of the reference's SDFTrainer without only_last (wisp/trainers/sdf_trainer.py:80-123):
    x_k = [position,] sum_{l <= k} blend_l ;  y_k = decoder(x_k) ;  S_k = sum_s (sdf_k - gt)^2 ;  R_k = sum_s |rgb_k - rgb_gt|^2
    loss = (sum_k w_sdf[k] S_k + sum_k w_rgb[k] R_k) inv_n ;  g_k = fl32((2 w[k]) diff_k [rgb (1 - rgb)] inv_n)
    every LOD's decoder backward is added into dW1, db1, dW2, db2; level l's table takes weight * sum_{k >= l} d features_k.
lods_reference writes that out directly; reference_by_cuts is the weighted sum over k of X.step_reference on the case cut to its first
k + 1 levels (the two agree wherever g does not round: on exact cases); autograd_reference is the reference's loop through the oracle.

Exact cases are X.build_case's: one target per sample, the FINEST LOD's float64 prediction plus a multiple of 1/4.  The coarser LODs
then differ from it by whatever the finer levels' blends add through W1 and w2 - multiples of the blends' quantum.  check_exact_lods
stacks the (LOD, sample) pairs as rows and finds one quantum per stage and output over all terms of all LODs, with fewer than 2^24
quanta: any order of addition is exact.  A refusal blames the inputs."""
import numpy as np
import torch

import sdf_step_exact_ref as X
import spc_exact_ref as S  # noqa: F401  (the cases are spc_exact_ref.make_case's)

F64 = torch.float64
C = X.C


def default_weights(case):
    """what SDFTrainStep passes: every distance term once; with colours LOD k's colour error L - k times (the running colour sum
    joins the loss inside the reference's LOD loop)"""
    L = len(case["levels"])
    return [1.0] * L, ([float(L - k) for k in range(L)] if case["tex"] else None)


def cut(case, k):
    """the case on its first k + 1 levels: what the one-LOD step sees when handed those levels"""
    out = dict(case)
    out["levels"] = tuple(case["levels"][:k + 1])
    out["tables"] = list(case["tables"][:k + 1])
    out["chain"] = case["chain"][:, :k + 1].contiguous()
    out["b"] = case["b"] + case["levels"][-1] - case["levels"][k]       # the samples keep their fraction bits (S.weights' grid)
    out.pop("report", None); out.pop("want", None)
    return out


def launch_shape(num_lods, n):
    """X.launch_shape: the all-LOD kernel keeps st_grid and the (sample, level) group mapping; idle groups idle in every phase"""
    return X.launch_shape(num_lods, n)


# ---------------------------------------------------------------------------------------------------- the float64 step
def lods_parts(case, w_sdf=None, w_rgb=None, gts=None, rgb_gts=None):
    """per LOD k the float64 forward and decoder backward: X.decoder_parts on the running sum of the blends, the LOD's weights in g"""
    n, tex, fo = case["n"], case["tex"], 3 if case["pos_input"] else 0
    L = len(case["levels"])
    dw_sdf, dw_rgb = default_weights(case)
    w_sdf = dw_sdf if w_sdf is None else w_sdf
    w_rgb = dw_rgb if w_rgb is None else w_rgb
    gts = (case["gts"] if gts is None else gts).double().reshape(-1)
    parts = X.level_parts(case)
    _, blends = X.features(case, parts)
    w1, b1, w2, b2 = (case[k].double() for k in ("w1", "b1", "w2", "b2"))
    inv_n = X.inv_n_of(n)
    lods, run = [], torch.zeros_like(blends[0])
    for k in range(L):
        run = run + blends[k]                                              # level order
        x = torch.cat([case["coords"].double(), run], 1) if fo else run
        a = x @ w1.T + b1
        h = torch.relu(a)
        y = h @ w2.T + b2
        d_sdf = y[:, -1] - gts
        if tex:
            col = (case["rgb_gts"] if rgb_gts is None else rgb_gts).double()
            rgb = X._sigmoid32(y[:, :3])
            d_rgb = rgb - col
            diff = torch.cat([d_rgb, d_sdf[:, None]], 1)
            g = torch.cat([(2.0 * w_rgb[k]) * d_rgb * (rgb * (1.0 - rgb)) * inv_n, ((2.0 * w_sdf[k]) * d_sdf * inv_n)[:, None]], 1)
        else:
            diff = d_sdf[:, None]
            g = (2.0 * w_sdf[k]) * diff * inv_n
        g_raw, g = g, g.float().double()
        gh = g[:, :, None] * w2[None, :, :]
        ga = torch.where(a > 0, gh.sum(1), torch.zeros_like(a))
        lods.append(dict(x=x, a=a, h=h, y=y, diff=diff, g=g, g_raw=g_raw, gh=gh, ga=ga, dfeat=X._mm(ga, w1[:, fo:])))
    return dict(parts=parts, blends=blends, lods=lods, fo=fo, inv_n=inv_n, w_sdf=list(w_sdf), w_rgb=None if w_rgb is None else list(w_rgb))


def _scatter(case, parts, dfeat_of_level):
    tables = []
    for l, ((w, rows, valid), t) in enumerate(zip(parts, case["tables"])):
        contrib = (w[:, :, None] * dfeat_of_level(l)[:, None, :])[valid]
        tables.append(torch.zeros(t.shape, dtype=F64).index_add_(0, rows[valid].reshape(-1), contrib.reshape(-1, C)))
    return tables


def lods_reference(case, w_sdf=None, w_rgb=None, gts=None, rgb_gts=None):
    """float64: dict(loss [1 + L] or [1 + 2L], tables, w1, b1, w2, b2, per_lod [L x the same gradients of LOD k alone])"""
    p = lods_parts(case, w_sdf, w_rgb, gts, rgb_gts)
    L, tex = len(case["levels"]), case["tex"]
    per = []
    for k, q in enumerate(p["lods"]):
        zero = torch.zeros_like(q["dfeat"])
        per.append(dict(tables=_scatter(case, p["parts"], lambda l: q["dfeat"] if l <= k else zero), w1=X._mm(q["ga"].T, q["x"]),
                        b1=q["ga"].sum(0), w2=X._mm(q["g"].T, q["h"]).reshape(case["w2"].shape), b2=q["g"].sum(0)))
    suffix = lambda l: sum(p["lods"][k]["dfeat"] for k in range(l, L))
    out = dict(tables=_scatter(case, p["parts"], suffix), per_lod=per, pred=[q["y"][:, -1] for q in p["lods"]])
    for name in ("w1", "b1", "w2", "b2"):
        out[name] = sum(d[name] for d in per)
    Sk = [(q["diff"][:, -1] ** 2).sum() for q in p["lods"]]
    Rk = [(q["diff"][:, :3] ** 2).sum() for q in p["lods"]] if tex else []
    total = sum(w * s for w, s in zip(p["w_sdf"], Sk)) + (sum(w * r for w, r in zip(p["w_rgb"], Rk)) if tex else 0.0)
    out["loss"] = torch.stack([total * p["inv_n"]] + Sk + Rk)
    return out


def reference_by_cuts(case, w_sdf=None, w_rgb=None):
    """the weighted sum over k of X.step_reference on cut(case, k).  With colours the two terms weigh differently: the distance
    term alone is the step whose colour targets are its own colours, the colour term alone the step whose distance targets are its
    own distances.  Equal to lods_reference wherever g does not round."""
    dw_sdf, dw_rgb = default_weights(case)
    w_sdf = dw_sdf if w_sdf is None else w_sdf
    w_rgb = dw_rgb if w_rgb is None else w_rgb
    L, tex = len(case["levels"]), case["tex"]
    acc = dict(tables=[torch.zeros(t.shape, dtype=F64) for t in case["tables"]])
    Sk, Rk, total = [], [], 0.0
    for k in range(L):
        c = cut(case, k)
        if tex:
            p = X.decoder_parts(c)
            own_rgb, own_sdf = X._sigmoid32(p["y"][:, :3]), p["y"][:, -1]
            terms = [(w_sdf[k], X.step_reference(c, rgb_gts=own_rgb)), (w_rgb[k], X.step_reference(c, gts=own_sdf))]
            Sk.append(terms[0][1]["loss"][1]); Rk.append(terms[1][1]["loss"][2])
            total = total + w_sdf[k] * Sk[-1] + w_rgb[k] * Rk[-1]
        else:
            terms = [(w_sdf[k], X.step_reference(c))]
            Sk.append(terms[0][1]["loss"][0] / X.inv_n_of(case["n"]))
            total = total + w_sdf[k] * Sk[-1]
        for w, r in terms:
            for l in range(k + 1):
                acc["tables"][l] = acc["tables"][l] + w * r["tables"][l]
            for name in ("w1", "b1", "w2", "b2"):
                acc[name] = acc.get(name, 0.0) + w * r[name]
    acc["loss"] = torch.stack([total * X.inv_n_of(case["n"])] + Sk + Rk)
    return acc


def autograd_reference(case, dtype=F64, w_sdf=None, w_rgb=None):
    """torch autograd through oracle.octree_grid.octree_grid_interpolate at lod_idx = k and the oracle's decoder, the reference's loop
    written out (sdf_trainer.py:80-123): with default weights the running colour sum joins the loss inside the loop"""
    from oracle import nerf as onerf, octree_grid as og
    tr, tex, H = case["tree"], case["tex"], case["w1"].shape[0]
    levels, n = list(case["levels"]), case["n"]
    L = len(levels)
    feats = [t.to(dtype).clone().requires_grad_(True) for t in case["tables"]]
    dec = onerf.OracleDecoder(case["w1"].shape[1], 4 if tex else 1, H, 1, True).to(dtype)
    with torch.no_grad():
        dec.layers[0].weight.copy_(case["w1"]); dec.layers[0].bias.copy_(case["b1"])
        dec.lout.weight.copy_(case["w2"].reshape(-1, H)); dec.lout.bias.copy_(case["b2"])
    gts = case["gts"].to(dtype).reshape(-1)
    loss, l2_loss, rgb_loss, Sk, Rk = 0.0, 0.0, 0.0, [], []
    for k in range(L):
        f = og.octree_grid_interpolate(tr.oracle_blas(), tr.trinkets, feats, case["coords"], k, 0, levels, 'sum', C, case["half_round"]).to(dtype)
        y = dec(torch.cat([case["coords"].to(dtype), f], 1) if case["pos_input"] else f)
        Sk.append(((y[:, -1] - gts) ** 2).sum())
        if tex:
            Rk.append(((torch.sigmoid(y[:, :3]) - case["rgb_gts"].to(dtype)) ** 2).sum())
        if w_sdf is None:
            if tex:
                rgb_loss = rgb_loss + Rk[-1]
                loss = loss + rgb_loss
            l2_loss = l2_loss + Sk[-1]
        else:
            loss = loss + w_sdf[k] * Sk[-1] + (w_rgb[k] * Rk[-1] if tex else 0.0)
    loss = (loss + l2_loss) / n
    loss.backward()
    zero = lambda t: torch.zeros_like(t) if t.grad is None else t.grad
    return dict(loss=torch.stack([loss] + Sk + Rk).detach(), tables=[zero(t) for t in feats], w1=dec.layers[0].weight.grad,
                b1=dec.layers[0].bias.grad, w2=dec.lout.weight.grad.reshape(case["w2"].shape), b2=dec.lout.bias.grad)


# ---------------------------------------------------------------------------------------------------- exactness
def _stack(p, key):
    return torch.cat([q[key] for q in p["lods"]], 0)


def check_exact_lods(case, w_sdf=None, w_rgb=None, prefill=X.PREFILL_MAX, forward_only=False):
    """X.check_exact_step over the rows of ALL LODs: one quantum per stage and output, fewer than 2^24 quanta in the absolute sum of
    all terms (and the pre-filled value).  Returns dict(spans, edge, nonzero_diff [per LOD], ...).
    forward_only stops once the forward of every LOD, the differences and g are known to be exact: what a case needs whose SUMS are
    then allowed to round (inexact_lods_case)."""
    n, tex = case["n"], case["tex"]
    L = len(case["levels"])
    assert n >= 1 and n & (n - 1) == 0, "n must be a power of two: 1 / n is exact"
    assert bool(torch.equal(case["gts"].float().double(), case["gts"].double())), "a target is no fp32 value"
    p = lods_parts(case, w_sdf, w_rgb)
    for w in p["w_sdf"] + (p["w_rgb"] or []):
        assert np.isfinite(w) and w > 0 and float(np.float32(w)) == w, "a weight is no positive fp32 value"
    fo = p["fo"]
    w1, b1, w2, b2 = (case[k].double() for k in ("w1", "b1", "w2", "b2"))
    spans = {}
    for li, ((w, rows, valid), t) in enumerate(zip(p["parts"], case["tables"])):
        t64 = t.half().double() if case["half_round"] else t.double()
        terms = (w[:, :, None] * t64[rows]) * valid[:, None, None]
        X._budget(f"blend{li}", terms.abs().sum(1), terms, spans)
        if case["half_round"]:
            raw = terms.sum(1)
            assert bool(torch.equal(raw.half().double(), raw)), f"level {case['levels'][li]}: a blend is no fp16 value"
    X._budget("features", sum(b.abs() for b in p["blends"]), torch.stack(p["blends"]), spans)      # (bounds every prefix)
    x, a, h, y, diff, g, gh, ga = (_stack(p, k) for k in ("x", "a", "h", "y", "diff", "g", "gh", "ga"))
    gts = case["gts"].double().reshape(-1).repeat(L)
    X._budget("a", x.abs() @ w1.abs().T + b1.abs(), torch.cat([x.reshape(-1), b1]), spans)
    s2 = h @ w2.abs().T + b2.abs()
    live_rows = [o for o in range(w2.shape[0]) if abs(float(b2[o])) != X.SAT_BIAS]
    X._budget("y", s2[:, live_rows] + gts.abs().reshape(-1, 1), torch.cat([h.reshape(-1), b2[live_rows], gts]), spans)
    if tex:
        with np.errstate(over="ignore"):
            e = np.exp(-y[:, :3].float().numpy())
        for o, mode in enumerate(case["modes"]):
            want = dict(half=1.0, low=np.inf, high=0.0)[mode]
            assert bool((e[:, o] == want).all()), f"colour {o} ({mode}): expf is not exactly {want} at every LOD"
            if mode != "half":
                assert float((h @ w2.abs().T)[:, o].max()) <= X.SAT_BIAS - 108.0, f"colour {o}: the row's sum can leave saturation"
        assert bool(torch.equal(case["rgb_gts"].float().double(), case["rgb_gts"].double()))
    assert bool(torch.equal(g, _stack(p, "g_raw"))), "inputs are not exact: g rounds"
    if forward_only:
        return dict(spans=spans)
    # the loss: S_k, R_k and the weighted total, over all rows
    sq = diff ** 2
    wrow_s = torch.tensor(p["w_sdf"], dtype=F64).repeat_interleave(n)
    weighted = [sq[:, -1] * wrow_s]
    if tex:
        weighted.append(sq[:, :3].sum(1) * torch.tensor(p["w_rgb"], dtype=F64).repeat_interleave(n))
        weighted.append(sq[:, :3].reshape(-1))
    X._budget("loss", sum(v.sum() for v in weighted[:2]).reshape(1), torch.cat([sq.reshape(-1)] + weighted), spans)
    X._budget("ga", gh.abs().sum(1), gh, spans)
    X._budget("b2", g.abs().sum(0), g, spans, prefill)
    X._budget("b1", ga.abs().sum(0), ga, spans, prefill)
    gr = g[:, :, None] * h[:, None, :]
    X._budget("w2", gr.abs().sum(0), gr, spans, prefill)
    X._budget("w1", ga.abs().T @ x.abs(), (ga[:, :, None] * x[:, None, :]).reshape(-1), spans, prefill)
    dfe_abs = ga.abs() @ w1.abs()[:, fo:]                                  # [L n, C]
    dfe_terms = ga[:, :, None] * w1[None, :, fo:]
    # the suffix sums: all terms of all LODs of a sample, in any order
    X._budget("dfeat", dfe_abs.reshape(L, n, C).sum(0), dfe_terms, spans)
    absmax, quanta, touched, touched_zero = 0.0, [], 0, 0
    for l, ((w, rows, valid), t) in enumerate(zip(p["parts"], case["tables"])):
        suf = sum(p["lods"][k]["dfeat"] for k in range(l, L))
        contrib = (w[:, :, None] * suf[:, None, :])[valid]
        assert bool(torch.equal(contrib.float().double(), contrib)), "a product weight * d features is no fp32 value"
        asum = torch.zeros(t.shape, dtype=F64).index_add_(0, rows[valid].reshape(-1), contrib.abs().reshape(-1, C))
        quanta.append(X._budget(f"table{l}", asum, contrib, spans, prefill))
        if valid.any():
            absmax = max(absmax, float((w[valid].max(1).values * suf[valid].abs().max(1).values).max()))
        total = torch.zeros(t.shape, dtype=F64).index_add_(0, rows[valid].reshape(-1), contrib.reshape(-1, C))
        touched += int((asum > 0).sum()); touched_zero += int(((asum > 0) & (total == 0)).sum())
    if absmax > 0:
        sh = X.sg_fixed_point_exponent(n, absmax)
        assert 2.0 ** -(sh - 1) <= min(quanta), "a table term is no multiple of the fixed-point quantum"
    edge = int(((a == 0) & (gh.abs().sum(1) != 0)).sum())
    nonzero = [int((q["diff"][:, -1] != 0).sum()) for q in p["lods"]]
    distinct = len({tuple(q["y"][:, -1].tolist()) for q in p["lods"]})
    return dict(spans=spans, edge=edge, nonzero_diff=nonzero, distinct_preds=distinct, table_touched=touched, table_zero=touched_zero,
                relu_both=bool((a > 0).any()) and bool((a < 0).any()))


_cases = {}


def exact_lods_case(tree_name, levels, n, hidden, w_sdf=None, w_rgb=None, **kw):
    """the first rung of X.LADDER at which X.build_case and check_exact_lods both accept; cached.  want = lods_reference."""
    key = (tree_name, tuple(levels), n, hidden, None if w_sdf is None else tuple(w_sdf), None if w_rgb is None else tuple(w_rgb),
           tuple(sorted(kw.items())))
    if key in _cases:
        return _cases[key]
    last = None
    for b, align in X.LADDER:
        if align > levels[-1]:
            continue
        try:
            case = X.build_case(tree_name, levels, n, hidden, b=b, align=align, **kw)
            rep = check_exact_lods(case, w_sdf, w_rgb)
        except AssertionError as e:
            last = e
            continue
        if not kw.get("all_miss"):
            assert 2 * rep["nonzero_diff"][-1] >= n, "fewer than half of the samples have a non-zero difference"
            if len(levels) > 1 and n >= 16:
                assert rep["distinct_preds"] > 1, "every LOD predicts the same"
        case = dict(case, report=rep, w_sdf=w_sdf, w_rgb=w_rgb)
        case["want"] = lods_reference(case, w_sdf, w_rgb)
        _cases[key] = case
        return case
    raise AssertionError(f"no exact all-LOD case for {key}: {last}")


def forward_exact_lods_case(tree_name, levels, n, hidden, **kw):
    """the first rung at which X.build_case accepts and the forward, the differences and g of EVERY LOD are exact: the base of
    inexact_lods_case where the full checker refuses the size (its sums may round there anyway)"""
    key = ("forward", tree_name, tuple(levels), n, hidden, tuple(sorted(kw.items())))
    if key in _cases:
        return _cases[key]
    last = None
    for b, align in X.LADDER:
        if align > levels[-1]:
            continue
        try:
            case = X.build_case(tree_name, levels, n, hidden, b=b, align=align, **kw)
            check_exact_lods(case, forward_only=True)
        except AssertionError as e:
            last = e
            continue
        _cases[key] = case
        return case
    raise AssertionError(f"no forward-exact all-LOD case for {key}: {last}")


# ---------------------------------------------------------------------------------------------------- derived bounds
U = X.U


def inexact_lods_case(case, n):
    """the first n samples of an exact or forward-exact case (X.inexact_case): only g's one rounding and the sums round"""
    out = X.inexact_case(case, n)
    out["want"] = lods_reference(out, case.get("w_sdf"), case.get("w_rgb"))
    return out


def derived_bounds(case, before):
    """X.derived_bounds over the rows of all LODs: per element (k + 2) 2^-24 A with k the number of non-zero terms of ALL LODs and A
    their absolute sum plus the pre-filled value.  A table element's terms are weight * (sum over k >= l of d features_k): the
    propagated error of that sum is (K + (L - l) + 1) 2^-24 times the absolute sum of its K leaf terms (the L - l chains, each leaf
    through at most its chain's roundings, then the L - l - 1 additions of the suffix sum), and one fixed-point quantum per
    contribution, doubled as in X."""
    p = lods_parts(case, case.get("w_sdf"), case.get("w_rgb"))
    n, fo, L, tex = case["n"], p["fo"], len(case["levels"]), case["tex"]
    x, a, h, g, gh, ga, diff = (_stack(p, k) for k in ("x", "a", "h", "g", "gh", "ga", "diff"))
    w1 = case["w1"].double()
    live = (a > 0).double()
    gh_live = gh * live[:, None, :]
    k_ga, a_ga = (gh_live != 0).double().sum(1), gh_live.abs().sum(1)
    nz = lambda t: (t != 0).double()
    out = {}
    k = k_ga.T @ nz(x); A = a_ga.T @ x.abs()
    out["w1"] = (k + 2) * U * (A + before["w1"].double().abs())
    out["b1"] = (k_ga.sum(0) + 2) * U * (a_ga.sum(0) + before["b1"].double().abs())
    k = torch.einsum("no,nh->oh", nz(g), nz(h)); A = torch.einsum("no,nh->oh", g.abs(), h)
    out["w2"] = ((k + 2) * U * (A + before["w2"].double().reshape(k.shape).abs())).reshape(case["w2"].shape)
    out["b2"] = (nz(g).sum(0) + 2) * U * (g.abs().sum(0) + before["b2"].double().abs())
    want = lods_reference(case, case.get("w_sdf"), case.get("w_rgb"))["loss"]
    lb = (n + 2) * U * want                                               # S_k, R_k: n squares each (all terms >= 0)
    lb[0] = ((2 if tex else 1) * n * L + 2 * L + 2) * U * want[0]          # every square, its product with the weight, the sums
    out["loss"] = lb
    k_df = (k_ga @ nz(w1[:, fo:])).reshape(L, n, C); a_df = (a_ga @ w1[:, fo:].abs()).reshape(L, n, C)
    absmax = 0.0
    sufs = []
    for l, (w, rows, valid) in enumerate(p["parts"]):
        suf = sum(p["lods"][kk]["dfeat"] for kk in range(l, L))
        sufs.append(suf)
        if valid.any():
            absmax = max(absmax, float((w[valid].max(1).values * suf[valid].abs().max(1).values).max()))
    quantum_fp = 2.0 * 2.0 ** -X.sg_fixed_point_exponent(n, absmax) if absmax > 0 else 0.0
    out["tables"] = []
    for l, ((w, rows, valid), t, bf) in enumerate(zip(p["parts"], case["tables"], before["tables"])):
        K = k_df[l:].sum(0); Aa = a_df[l:].sum(0)
        e_suf = (K + (L - l) + 1) * U * Aa
        r = rows[valid].reshape(-1)
        add = lambda v: torch.zeros(t.shape, dtype=F64).index_add_(0, r, v.reshape(-1, C))
        contrib = (w[:, :, None] * sufs[l][:, None, :])[valid]
        k = add(nz(contrib)); A = add(contrib.abs())
        prop = add((w[:, :, None] * e_suf[:, None, :])[valid])
        out["tables"].append((k + 2) * U * (A + bf.double().abs()) + prop * (1 + (k + 2) * U) + k * quantum_fp)
    return out


# ---------------------------------------------------------------------------------------------------- the cases of the GPU file
# (tree, levels) -> (samples per pass, idle groups): 1 -> (16, 0), 2 -> (8, 0), 3 -> (5, 1), 6 -> (2, 4), 8 -> (2, 0), 9 -> (1, 7)
LEVEL_LISTS = (("small", (5,)), ("small", (4, 5)), ("small", (3, 4, 5)), ("small", (0, 1, 2, 3, 4, 5)),
               ("deep", (1, 2, 3, 4, 5, 6, 7, 8)), ("deep", (2, 3, 4, 5, 6, 7, 8, 9, 10)))
COVERAGE = {1: (16, 0), 2: (8, 0), 3: (5, 1), 6: (2, 4), 8: (2, 0), 9: (1, 7)}
NS = (1, 2, 16, 64, 512)
# 9 levels: 1 sample per pass, 1024 workgroups, two passes each.  The plain field only: with colours check_exact_lods refuses n = 2048
# at every rung (the weighted loss total needs 24.8 bits); the textured field's second pass is INEXACT_BIG's, in the bounded test.
TWO_PASS = ("deep", (2, 3, 4, 5, 6, 7, 8, 9, 10), 2048)
HIDDENS = (1, 17, 128, 256)
INEXACT_NS = (37, 513)
INEXACT_BIG = ("small", (0, 1, 2, 3, 4, 5), 2049)
