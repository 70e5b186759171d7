"""Host: the builders and float64 references of tests/composite_exact_ref.py against the oracle (oracle.render with autograd, the
trainer's loss of multiview_trainer.py:140-154), so that a mismatch in tests/test_gpu_composite_exact.py is the kernel's."""
import numpy as np
import pytest
import torch

import composite_exact_ref as R
from oracle import render as orender

FLAGS = [(True, True, True), (False, True, True), (True, False, False), (False, False, False)]


def _oracle(c, dtype, flags, g_rgb, g_alpha, g_depth):
    """oracle.render.composite with autograd -> every output and both gradients, as float64 numpy"""
    with_depths, with_alpha, with_depth_grad = flags
    S, R_ = c["S"], c["R"]
    t = lambda a: torch.from_numpy(np.asarray(a, np.float64)).to(dtype)
    color, density = t(c["color"]).requires_grad_(True), t(np.reshape(c["density"], (S, 1))).requires_grad_(True)
    ridx = torch.from_numpy(c["ray"].astype(np.int64))
    boundary = torch.ones(S, dtype=torch.bool)
    boundary[1:] = ridx[1:] != ridx[:-1]
    out = orender.composite(color, density, t(np.reshape(c["delta"], (S, 1))), t(c["depths"]), ridx, boundary, R_,
                            np.float32(c["bg"]).astype(np.float64), with_depth=with_depths)
    loss = (out["rgb"] * t(g_rgb)).sum()
    if with_alpha:
        loss = loss + (out["alpha"] * t(g_alpha)).sum()
    if with_depths and with_depth_grad:
        loss = loss + (out["depth"] * t(g_depth)).sum()
    loss.backward()
    res = dict(rgb=out["rgb"], alpha=out["alpha"], weights=out["weights"], grad_color=color.grad, grad_density=density.grad)
    if with_depths:
        res["depth"] = out["depth"]
    res = {k: v.detach().double().numpy() for k, v in res.items()}
    res["hit"] = out["hit"].numpy()
    return res


def _oracle_by_groups(c, flags):
    """the oracle takes a pack's sums as differences of one running sum over ALL samples, so a ray behind the one whose tau adds up
    to 2 457 would carry that ray's float64 rounding: that ray goes through the oracle on its own"""
    dense = [R.B_DENSE_RAY] if c["name"] == "main" else []
    groups = [np.array([r for r in range(c["R"]) if r not in dense])] + ([np.array(dense)] if dense else [])
    whole = {}
    for rays in groups:
        sel = np.isin(c["ray"], rays)
        sub = dict(c, R=len(rays), S=int(sel.sum()), ray=np.searchsorted(rays, c["ray"][sel]))
        for n in ("color", "density", "delta", "depths"):
            sub[n] = c[n][sel]
        res = _oracle(sub, torch.float64, flags, c["g_rgb"][rays], c["g_alpha"][rays], c["g_depth"][rays])
        for n, v in res.items():
            per_ray = n in ("rgb", "alpha", "depth", "hit")
            if n not in whole:
                whole[n] = np.zeros(((c["R"] if per_ray else c["S"]),) + v.shape[1:], v.dtype)
            whole[n][rays if per_ray else sel] = v
    return whole


@pytest.mark.parametrize("name", R.BWD_NAMES)
def test_family_a_reference_equals_oracle_in_fp32_and_float64(name):
    """the builder's assertions hold, and oracle.render.composite with autograd gives the reference's bits in fp32 and in float64"""
    c = R.bwd_case(name)
    for flags in (FLAGS if name != "sweep1024" else FLAGS[:1]):
        want = R.reference_bwd(c, *flags)
        for dtype in (torch.float32, torch.float64):
            got = _oracle(c, dtype, flags, c["g_rgb"], c["g_alpha"], c["g_depth"])
            for n, v in got.items():
                w = want[n].numpy()
                assert np.array_equal(v, w.astype(v.dtype)), (name, flags, dtype, n, int((v != w).sum()))


@pytest.mark.parametrize("name", sorted(R.SPEC_LISTS))
def test_family_a_loss_reference_equals_oracle_and_trainer_loss(name):
    """float64 autograd through the oracle and the trainer's loss, taken as a SUM so that its gradient is dyadic: rgb bit for bit, the
    sum of the loss terms, d / d colour and d / d density before the factor inv_n.  What the reference adds on top is the one fp32
    subtraction and the roundings by inv_n that its docstring states."""
    c = R.loss_case(name)
    for kind in R.KINDS:
        want = R.reference_loss(c, kind)
        S = c["S"]
        t = lambda a: torch.from_numpy(np.asarray(a, np.float64))
        color, density = t(c["color"]).requires_grad_(True), t(np.reshape(c["density"], (S, 1))).requires_grad_(True)
        ridx = torch.from_numpy(c["ray"].astype(np.int64))
        boundary = torch.ones(S, dtype=torch.bool)
        boundary[1:] = ridx[1:] != ridx[:-1]
        delta = t(np.reshape(c["delta"], (S, 1)))
        out = orender.composite(color, density, delta, delta, ridx, boundary, c["R"], c["bg"], with_depth=False)
        x = out["rgb"] - t(c["gt"])
        if kind == "huber":
            per = torch.where(x.abs() < 1.0, 0.5 * x * x, x.abs() - 0.5)
        else:
            per = x * x if kind == "l2" else x.abs()
        per.sum().backward()
        assert np.array_equal(out["rgb"].detach().numpy(), want["rgb"].double().numpy())
        assert float(per.sum().detach()) == want["loss_sum"]
        assert np.array_equal(color.grad.numpy(), want["grad_color_unit"])
        assert np.array_equal(density.grad.numpy()[:, 0], want["grad_density_unit"])
        # the loss: fl(fl(sum) * inv_n) lies within two roundings of the float64 mean
        mean = float(per.mean().detach())
        assert abs(float(want["loss"]) - mean) <= 2.0 ** -22 * abs(mean)
        # the fp32 outputs are the unit quantities times inv_n, to the one rounding each
        inv_n = float(want["inv_n"])
        gd = want["grad_density"].double().numpy()[:, 0]
        assert np.all(np.abs(gd - want["grad_density_unit"] * inv_n) <= 2.0 ** -23 * np.abs(want["grad_density_unit"]).max() * inv_n * 2)
        assert np.array_equal(want["grad_color"].double().numpy(), want["grad_color_unit"] * inv_n)


def test_family_a_shares_and_sweep_slots():
    total = nonzero = 0
    for name in R.BWD_NAMES:
        c = R.bwd_case(name)
        want = R.reference_bwd(c)
        assert want["zero_share"] <= 0.10
        total += c["S"]
        nonzero += want["nonzero"]
        print(f"bwd {name}: R = {c['R']}, S = {c['S']}, non-zero grad_density {want['nonzero'] / c['S']:.1%}, zero leading samples {want['zero_share']:.1%}")
    for name in R.LOSS_NAMES:
        c = R.loss_case(name)
        want = R.reference_loss(c, "huber")
        assert want["zero_share"] <= 0.10
        total += c["S"]
        nonzero += want["nonzero"]
        print(f"loss {name}: R = {c['R']}, S = {c['S']}, non-zero grad_density {want['nonzero'] / c['S']:.1%}, zero leading samples {want['zero_share']:.1%}")
    assert nonzero >= 0.25 * total, (nonzero, total)
    # every (chunk, lane) slot of the 1024 sweep carries the weight exactly once; four consecutive rays are all long
    for name, n in (("sweep1024", 1024), ("sweep256", 256)):
        c = R.loss_case(name)
        assert np.all(c["lens"] == n) and c["R"] == n
        slots = sorted((int(k) // 64, int(k) % 64) for k in c["k"])
        assert slots == [(ch, ln) for ch in range(n // 64) for ln in range(64)]
    # the lengths of Family B begin with those of tests/test_gpu_composite_split.py
    import test_gpu_composite_split as split
    assert R.B_LENS[:len(split.LENS)] == split.LENS and (R.B_ZERO_RAY, R.B_DENSE_RAY) == (split.ZERO_RAY, split.DENSE_RAY)
    assert all(n in R.B_LENS for n in (1023, 1024, 1025, 4000))
    main = R.main_specs()
    for n in R.LENGTHS:
        assert {k for m, k in main if m == n} >= set(R.positions(n))
    assert R.loss_case("stride37")["R"] == 37 and R.loss_case("stride4099")["R"] == 4099


@pytest.mark.parametrize("name,channels,lens", R.PACK_CASES, ids=[p[0] for p in R.PACK_CASES])
def test_family_a_packed_reference_equals_oracle(name, channels, lens):
    p = R.packed_case(channels, lens)
    feats, boundary = torch.from_numpy(p["feats"]), torch.from_numpy(p["boundary"])
    assert p["S"] == sum(lens) and (not lens or p["starts"][-1] + lens[-1] == p["S"])        # the last pack ends at num_samples
    assert torch.equal(orender.sum_reduce(feats, boundary).float(), R.reference_sum_reduce(p))
    for exclusive in (False, True):
        assert torch.equal(orender.cumsum(feats, boundary, exclusive=exclusive).float(), R.reference_cumsum(p, exclusive, False))
        # reverse, from the contract: the running sum of the pack read backwards
        rev = R.reference_cumsum(p, exclusive, True).numpy()
        for b, n in zip(p["starts"], lens):
            seg = p["feats"][b:b + n][::-1]
            want = np.cumsum(seg, 0) - (seg if exclusive else 0)
            assert np.array_equal(rev[b:b + n], want[::-1])


@pytest.mark.parametrize("name", ["main", "tail2", "three"])
def test_family_b_reference_agrees_with_float64_autograd(name):
    c = R.b_case(name)
    tt = np.bincount(c["ray"], weights=(c["density"].astype(np.float64) * c["delta"])[:, 0], minlength=c["R"])
    if name == "main":
        assert tt[R.B_ZERO_RAY] == 0 and np.float32(np.exp(-tt[R.B_DENSE_RAY])) == 0.0
        rest = np.delete(tt, [R.B_ZERO_RAY, R.B_DENSE_RAY])
        assert rest[rest > 0].min() >= 0.99 and rest.max() <= 12.01
    for flags in FLAGS:
        ref, scale, scale_e = R.reference_b(c, c["g_rgb"], c["g_alpha"] if flags[1] else None, c["g_depth"] if flags[2] else None, flags[0])
        got = _oracle_by_groups(c, flags)
        for n, v in got.items():
            if n == "hit":
                assert np.array_equal(v, ref[n])
                continue
            err = np.abs(v - ref[n]).max() if v.size else 0.0
            assert err <= 1e-12 * max(np.abs(ref[n]).max(), 1e-300), (name, flags, n, err)
            assert np.all(scale[n] >= 0) and np.all(scale_e[n] >= scale[n])
    # the fused loss: float64 autograd through the oracle and the trainer's mean loss
    for kind in R.KINDS:
        ref = R.reference_b_loss(c, kind)[0]
        S = c["S"]
        t = lambda a: torch.from_numpy(np.asarray(a, np.float64))
        color, density = t(c["color"]).requires_grad_(True), t(c["density"]).requires_grad_(True)
        ridx = torch.from_numpy(c["ray"].astype(np.int64))
        boundary = torch.ones(S, dtype=torch.bool)
        boundary[1:] = ridx[1:] != ridx[:-1]
        out = orender.composite(color, density, t(c["delta"]), t(c["delta"]), ridx, boundary, c["R"], np.float32(c["bg"]).astype(np.float64),
                                with_depth=False)
        x = out["rgb"] - t(c["gt"])
        if kind == "huber":
            per = torch.where(x.abs() < 1.0, 0.5 * x * x, x.abs() - 0.5)
        else:
            per = x * x if kind == "l2" else x.abs()
        per.mean().backward()
        assert abs(float(per.mean().detach()) - ref["loss"]) <= 1e-12 * abs(ref["loss"])
        for n, v in (("grad_color", color.grad.numpy()), ("grad_density", density.grad.numpy()), ("rgb", out["rgb"].detach().numpy())):
            assert np.abs(v - ref[n]).max() <= 1e-12 * np.abs(ref[n]).max(), (name, kind, n)
