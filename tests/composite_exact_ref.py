"""Builders and float64 references of the exact-arithmetic compositing tests (host only; test infrastructure).

Family A - inputs on which compositing (csrc/render.hip) has no rounding at all.  A sample's tau = density * delta is exactly 0
(density 0, delta a power of two in [2^-3, 2]: expf(-0) = 1) or exactly 1024 (density 1024 / delta: expf(-1024) = 0 in fp32 AND in
float64).  A ray has k leading transparent samples (T = 1, et = 1, w = 0), optionally one first opaque sample (w = 1 exactly) and
trailing samples of both kinds (T = 0, w = 0); every running sum of tau is a multiple of 1024 below 2^24.  So `weights` is one-hot
per ray, alpha is 0 or 1, rgb is bg or the colour of the first opaque sample, grad_color is g_rgb at that sample, and
grad_density = (G_i - G_k) delta_i on the leading samples (G_i delta_i on rays without an opaque sample) and exactly 0 from the
opaque sample on - a lost carry of the suffix sums leaves +-G_k there.
  * composite_fwd / composite_bwd ("bwd" cases): colours, depths and upstream gradients are small integers, bg is dyadic, so every G
    is an exact dyadic in any order and under any contraction.
  * composite_loss ("loss" cases): the kernel forms g_c = d_c inv_n with inv_n = fl(1 / (3 R)), not dyadic.  gt = rgb - x with x zero or
    a signed power of two (|x| on both sides of 1), so d_c is zero or a signed power of two for huber, l2 and l1 and g_c is exact;
    colours are bg plus zero or a signed power of two in ONE channel, or the same offset in two channels whose x are equal, so
    p0 + p1 and (p0 + p1) + p2 are inv_n times zero or a signed power of two however they are contracted.  The one rounding left is
    the subtraction G_i - G_k, a single IEEE operation contracted or not; the reference does it once in fp32.  The loss is
    fl(sum * inv_n) with an exact sum of dyadic terms; the reference applies that rounding explicitly too.
The builders assert their own conditions (a failing assertion here means bad inputs, not a wrong kernel): every value the kernels
round equals its fp32 round trip, at most 10 % of the leading samples expect a grad_density of exactly 0, every ray with an opaque
sample has G_k != 0.

Family A' - packed_sum_reduce / packed_cumsum only add: integer features in [-4, 4] make them exact.  `reverse` is stated from the
kernel's contract (the oracle has none): a running sum from the pack's last sample backwards.

Family B - realistic magnitudes: a float64 reference per ray, evaluated from the fp32 inputs and written from the formulas in the
header comment of composite_bwd_kernel, with the per-element error scale A_i of tests/test_gpu_composite_exact.py.
tests/test_composite_exact_host.py pins all three to oracle.render.
"""
import numpy as np
import torch

BG = (0.25, -0.5, 2.0)                       # dyadic
BG_B = (0.2, 0.5, 0.9)
LENGTHS = [0, 1, 2, 63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256, 257, 511, 512, 513, 718, 1023, 1024, 1025, 2047, 2048, 2049,
           4000]
FIXED_POS = (62, 63, 64, 65, 127, 128, 255, 256, 257, 1023)
NONE = -1
KINDS = ("huber", "l2", "l1")
F32_EPS = 2.0 ** -24
TINY = 2.0 ** -120          # Family B: a difference this small is not counted - below fp32's normal range (2^-126, times an upstream
                            # gradient of at most 2^6) a value has an absolute spacing, no relative precision


def positions(n):
    """where the one opaque sample of a ray of n samples sits: none, 0, n - 1, n / 2 and the chunk edges that fit"""
    if n == 0:
        return [NONE]
    out = []
    for p in [NONE, 0, n - 1, n // 2] + [p for p in FIXED_POS if p < n]:
        if p not in out:
            out.append(p)
    return out


def main_specs():
    """(length, opaque position) per ray.  Four consecutive rays share a workgroup of the split kernel; behind the length x
    position list come the workgroups whose composition matters, and one long ray alone in the last workgroup (R % 4 == 1)."""
    specs = [(n, k) for n in LENGTHS for k in positions(n)]
    specs += [(0, NONE)] * (-len(specs) % 4)
    specs += [(0, NONE), (0, NONE), (0, NONE), (1024, 1023),          # the long ray on wave 3, nothing on waves 0 to 2
              (5, 2), (300, 299), (2049, 100), (700, 64),             # short, long and over-long in one workgroup
              (1025, 1024), (40, NONE), (1024, 0), (64, 63),
              (4000, 3999), (718, 717), (65, 64), (1, 0),
              (600, 599)]
    assert len(specs) % 4 == 1
    return specs


SPEC_LISTS = {
    "main": main_specs,
    "tail2": lambda: [(3, 1), (70, 69), (0, NONE), (128, 64), (10, NONE), (513, 512)],                  # R % 4 == 2, the last ray long
    "tail3": lambda: [(3, 1), (70, 69), (0, NONE), (128, 64), (10, NONE), (64, 0), (1024, 1000)],       # R % 4 == 3
    "one": lambda: [(333, 200)],                                                                        # R < 4
    "two": lambda: [(0, NONE), (129, 128)],
    "three": lambda: [(7, 3), (333, 332), (0, NONE)],
    "sweep1024": lambda: [(1024, j) for j in range(1024)],         # every (chunk, lane) slot of the split kernel carries the weight once
    "sweep256": lambda: [(256, j) for j in range(256)],
    "stride37": lambda: [(n, k) for n in (0, 1, 2, 63, 64, 65, 130, 257) for k in positions(n)][:37],
    "stride4099": lambda: [(n, NONE if j % 5 == 0 else n // 2) for j in range(4099) for n in [1 + (7 * j) % 90 if j % 500 else 700]],
}
BWD_NAMES = ("main", "tail2", "three", "sweep256", "sweep1024")
LOSS_NAMES = ("main", "tail2", "tail3", "one", "two", "three", "sweep1024")
WORKER_LOSS_NAMES = ("main", "tail2", "tail3", "one", "two", "three")      # what the WISP_COMPOSITE_WAVES children run
_cases = {}


def _is_f32(a):
    a = np.asarray(a, np.float64)
    return bool(np.array_equal(a.astype(np.float32).astype(np.float64), a))


def _pow2_or_zero(a):
    a = np.abs(np.asarray(a, np.float64))
    m, _ = np.frexp(a)
    return bool(np.all((a == 0) | (m == 0.5)))


def _layout(specs, rng):
    lens = np.array([n for n, _ in specs], np.int64)
    k = np.array([p for _, p in specs], np.int64)
    assert np.all((k < lens) & (k >= NONE))
    R = len(specs)
    offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    S = int(offs[-1])
    ray = np.repeat(np.arange(R), lens)
    pos = np.arange(S) - offs[ray]
    kk = np.where(k < 0, np.int64(1) << 40, k)[ray]
    lead, first, trail = pos < kk, pos == kk, pos > kk
    opaque = first | (trail & (rng.uniform(size=S) < 0.5))
    delta = 2.0 ** rng.integers(-3, 2, S)                                            # [2^-3, 2]
    density = np.where(opaque, 1024.0 / delta, 0.0)
    tau = density * delta
    assert np.all((tau == 0) | (tau == 1024.0)) and (S == 0 or np.bincount(ray, weights=tau, minlength=R).max() < 2 ** 24)
    has = k >= 0
    return dict(R=R, S=S, lens=lens, k=k, offs=offs, ray=ray, pos=pos, lead=lead, first=first, has=has, idx_k=(offs[:-1] + k)[has],
                delta=delta, density=density)


def _finish(case, arrays):
    for name in arrays:
        assert _is_f32(case[name]), f"{case['name']}: {name} is not exact in fp32"
    return case


def bwd_case(name):
    """inputs of composite_fwd / composite_bwd in ray-offset mode (float64 arrays holding fp32 values)"""
    key = ("bwd", name)
    if key in _cases:
        return _cases[key]
    rng = np.random.default_rng(4100 + sorted(SPEC_LISTS).index(name))
    c = _layout(SPEC_LISTS[name](), rng)
    R, S, ray = c["R"], c["S"], c["ray"]
    color = rng.integers(-4, 5, (S, 3)).astype(np.float64)
    depths = rng.integers(1, 9, (S, 1)).astype(np.float64)
    g_rgb = rng.integers(-3, 4, (R, 3)).astype(np.float64)
    g_rgb[np.all(g_rgb == 0, axis=1), 0] = 1.0
    g_alpha = rng.integers(-2, 3, (R, 1)).astype(np.float64)
    g_depth = rng.integers(-2, 3, (R, 1)).astype(np.float64)
    c.update(name=name, color=color, depths=depths, g_rgb=g_rgb, g_alpha=g_alpha, g_depth=g_depth, bg=BG)
    # G_k != 0 under each of the four (grad_alpha, grad_depth) selections: move the opaque sample's colour along a channel with g != 0
    ch = np.argmax(g_rgb != 0, axis=1)
    for _ in range(40):
        bad = np.zeros(R, bool)
        for wa in (False, True):
            for wd in (False, True):
                G = _G_bwd(c, wa, wd)
                bad[np.nonzero(c["has"])[0][G[c["idx_k"]] == 0]] = True
        if not bad.any():
            break
        rows = (c["offs"][:-1] + c["k"])[bad]
        color[rows, ch[bad]] += 1.0
    assert not bad.any()
    _cases[key] = _finish(c, ("color", "depths", "g_rgb", "g_alpha", "g_depth", "delta", "density"))
    return c


def _G_bwd(c, with_alpha, with_depth):
    ray = c["ray"]
    G = (c["g_rgb"][ray] * (c["color"] - np.array(c["bg"]))).sum(1)
    if with_alpha:
        G = G + c["g_alpha"][ray, 0]
    if with_depth:
        G = G + c["g_depth"][ray, 0] * c["depths"][:, 0]
    return G


def _lead_density_grad(c, G, sub=None):
    """(G_i - G_k) delta_i on the leading samples, 0 from the opaque sample on; checks the builder's two conditions on G"""
    Gk = np.zeros(c["R"])
    Gk[c["has"]] = G[c["idx_k"]]
    assert np.all(Gk[c["has"]] != 0), f"{c['name']}: a ray's G_k is 0"
    diff = (G - Gk[c["ray"]]) if sub is None else sub(G, Gk[c["ray"]])
    gd = np.where(c["lead"], diff * c["delta"], 0.0)
    n_lead = int(c["lead"].sum())
    zero_share = float((gd[c["lead"]] == 0).mean()) if n_lead else 0.0
    assert zero_share <= 0.10, f"{c['name']}: {zero_share:.3f} of the leading samples expect a zero grad_density"
    return gd, zero_share


def _t32(a, shape=None):
    a = np.asarray(a, np.float64)
    assert _is_f32(a)
    t = torch.from_numpy(a.astype(np.float32))
    return t if shape is None else t.reshape(shape)


def reference_bwd(c, with_depths=True, with_alpha=True, with_depth_grad=True):
    """every output of composite_fwd and composite_bwd as fp32 tensors.  grad_depth acts only together with depths."""
    R, S = c["R"], c["S"]
    bg = np.array(c["bg"])
    wd = with_depths and with_depth_grad
    G = _G_bwd(c, with_alpha, wd)
    gd, zero_share = _lead_density_grad(c, G)
    w = c["first"].astype(np.float64)
    rgb = np.tile(bg, (R, 1))
    rgb[c["has"]] = c["color"][c["idx_k"]]
    alpha = c["has"].astype(np.float64)
    depth = np.zeros(R)
    depth[c["has"]] = c["depths"][c["idx_k"], 0]
    out = dict(rgb=_t32(rgb), alpha=_t32(alpha, (R, 1)), hit=torch.from_numpy(c["has"].copy()), weights=_t32(w, (S, 1)),
               grad_color=_t32(w[:, None] * c["g_rgb"][c["ray"]]), grad_density=_t32(gd, (S, 1)), zero_share=zero_share,
               nonzero=int((gd != 0).sum()))
    out["depth"] = _t32(depth, (R, 1)) if with_depths else None
    return out


def pack_mode(c, seed=5):
    """the same samples as packs with a `ridx` per sample: the packs' rays come in a shuffled, non-monotone order, rays without
    samples own no pack (and three more rays are added that own none); the last pack ends at num_samples.
    -> dict(ridx [S], starts [P], num_rays, new_of_ray [R])"""
    R2 = c["R"] + 3
    nonempty = c["lens"] > 0
    while True:                                      # (two packs can come out in rising order by chance)
        new_of_ray = np.random.default_rng(seed).permutation(R2)[:c["R"]]
        if nonempty.sum() < 2 or np.any(np.diff(new_of_ray[nonempty]) < 0):
            break
        seed += 1
    return dict(ridx=new_of_ray[c["ray"]].astype(np.int64), starts=c["offs"][:-1][nonempty].astype(np.int64), num_rays=R2,
                new_of_ray=new_of_ray)


def scatter_rays(t, pm, fill):
    """a per-ray tensor of the ray-offset order in the order of pack_mode; rays that own no pack hold `fill`"""
    out = torch.empty((pm["num_rays"],) + tuple(t.shape[1:]), dtype=t.dtype)
    out[:] = torch.as_tensor(fill, dtype=t.dtype)
    out[torch.from_numpy(pm["new_of_ray"])] = t
    return out


# ---------------------------------------------------------------------------------------------------- composite_loss
XS = np.array([0.0, 0.25, -0.25, 0.5, -0.5, 1.0, -1.0, 2.0, -2.0])


def loss_case(name):
    key = ("loss", name)
    if key in _cases:
        return _cases[key]
    rng = np.random.default_rng(5200 + sorted(SPEC_LISTS).index(name))
    c = _layout(SPEC_LISTS[name](), rng)
    R, S, ray = c["R"], c["S"], c["ray"]
    bg = np.array(BG)
    x = XS[rng.integers(0, len(XS), (R, 3))]
    x = np.where((x == 0) & (rng.uniform(size=(R, 3)) < 0.7), XS[rng.integers(1, len(XS), (R, 3))], x)
    pair = rng.uniform(size=R) < 0.4
    x[pair, 1] = x[pair, 0]
    allzero = np.all(x == 0, axis=1)
    x[allzero, rng.integers(0, 3, int(allzero.sum()))] = XS[rng.integers(1, len(XS), int(allzero.sum()))]
    pair = (x[:, 0] == x[:, 1]) & (x[:, 0] != 0)
    # one non-zero channel per sample (or none), or channels 0 and 1 alike on a ray whose x_0 = x_1
    off = np.zeros((S, 3))
    val = rng.choice([-1.0, 1.0], S) * 2.0 ** rng.integers(-6, 6, S)
    chan = rng.integers(0, 3, S)
    live = rng.uniform(size=S) >= 0.05
    off[np.arange(S)[live], chan[live]] = val[live]
    both = pair[ray] & (rng.uniform(size=S) < 0.3)
    off[both, 0] = val[both]; off[both, 1] = val[both]; off[both, 2] = 0.0
    # the opaque sample: its one offset on the first channel with x != 0, so that G_k != 0
    if c["idx_k"].size:
        rk = np.nonzero(c["has"])[0]
        off[c["idx_k"]] = 0.0
        off[c["idx_k"], np.argmax(x[rk] != 0, axis=1)] = val[c["idx_k"]]
    color = bg + off
    rgb = np.tile(bg, (R, 1))
    rgb[c["has"]] = color[c["idx_k"]]
    c.update(name=name, color=color, off=off, x=x, rgb=rgb, gt=rgb - x, bg=BG)
    assert np.array_equal(color - bg, off) and np.array_equal(rgb - c["gt"], x)
    _cases[key] = _finish(c, ("color", "gt", "rgb", "delta", "density"))
    return c


def loss_terms(x, kind):
    """(per-element loss, d loss / d x without the 1 / N) of MultiviewTrainer.step (multiview_trainer.py:140-154)"""
    a = np.abs(x)
    if kind == "huber":
        return np.where(a < 1.0, 0.5 * x * x, a - 0.5), np.clip(x, -1.0, 1.0)
    if kind == "l2":
        return x * x, 2.0 * x
    return a, np.sign(x)


def reference_loss(c, kind):
    """loss, grad_color, grad_density, rgb of wisp_composite_loss as fp32 tensors, plus the unit quantities (before inv_n) that the
    host test holds to float64 autograd"""
    R, S, ray = c["R"], c["S"], c["ray"]
    l, d = loss_terms(c["x"], kind)
    assert _pow2_or_zero(d)
    inv_n = np.float32(1.0) / np.float32(3 * R)
    u = d[ray] * c["off"]                                                 # p_c / inv_n, exact
    for s in (u[:, 0] + u[:, 1], (u[:, 0] + u[:, 1]) + u[:, 2], u[:, 1] + u[:, 2], u[:, 0] + u[:, 2]):
        assert _pow2_or_zero(s), f"{c['name']}: a partial sum of G is not inv_n times a power of two"
    Gu = u.sum(1)
    g = d * np.float64(inv_n)
    G = Gu * np.float64(inv_n)
    assert _is_f32(g) and _is_f32(G)
    G32 = G.astype(np.float32)
    gd, zero_share = _lead_density_grad(c, G32, sub=lambda a, b: (a - b.astype(np.float32)).astype(np.float64))        # ONE fp32 subtraction
    assert G32.dtype == np.float32 and _is_f32(gd)
    gd_unit, _ = _lead_density_grad(c, Gu)
    w = c["first"].astype(np.float64)
    # the sum of the loss terms is exact in fp32 in any order: all are multiples of `unit`, and their total stays below 2^24 units
    nz = l[l != 0]
    unit = 2.0 ** np.floor(np.log2(np.abs(nz).min())) if nz.size else 1.0
    while not np.array_equal(np.round(l / unit), l / unit):
        unit /= 2.0
    assert np.abs(l).sum() / unit < 2 ** 24
    total = l.sum()
    loss = np.float32(np.float32(total) * inv_n)
    return dict(loss=torch.tensor([loss], dtype=torch.float32), grad_color=_t32(w[:, None] * g[ray]), grad_density=_t32(gd, (S, 1)),
                rgb=_t32(c["rgb"]), inv_n=inv_n, d=d, loss_sum=total, grad_color_unit=w[:, None] * d[ray],
                grad_density_unit=gd_unit, zero_share=zero_share, nonzero=int((gd != 0).sum()))


# ---------------------------------------------------------------------------------------------------- Family A': packed primitives
PACK_LENGTHS = [1, 2, 63, 64, 65, 128, 129, 1000, 5000]
PACK_CHANNELS = (1, 3, 4, 7)
PACK_CASES = [(f"c{C}", C, PACK_LENGTHS[i:] + PACK_LENGTHS[:i]) for i, C in enumerate(PACK_CHANNELS)] + \
             [("zero-packs", 3, []), ("one-pack", 4, [65])]


def packed_case(channels, lens, seed=77):
    rng = np.random.default_rng(seed + channels)
    starts = np.concatenate([[0], np.cumsum(lens)])[:-1].astype(np.int64) if lens else np.zeros(0, np.int64)
    S = int(sum(lens))
    feats = rng.integers(-4, 5, (S, channels)).astype(np.float64)
    boundary = np.zeros(S, bool)
    boundary[starts] = True
    return dict(feats=feats, starts=starts, boundary=boundary, S=S, lens=list(lens), channels=channels)


def reference_sum_reduce(p):
    out = np.zeros((len(p["lens"]), p["channels"]))
    for i, (b, n) in enumerate(zip(p["starts"], p["lens"])):
        for j in range(b, b + n):
            out[i] += p["feats"][j]
    return _t32(out)


def reference_cumsum(p, exclusive, reverse):
    """per pack a running sum from its first sample on - with `reverse` from its last sample backwards; `exclusive` leaves a
    sample's own value out"""
    out = np.zeros_like(p["feats"])
    for b, n in zip(p["starts"], p["lens"]):
        run = np.zeros(p["channels"])
        order = range(b + n - 1, b - 1, -1) if reverse else range(b, b + n)
        for j in order:
            if exclusive:
                out[j] = run
            run = run + p["feats"][j]
            if not exclusive:
                out[j] = run
    return _t32(out)


# ---------------------------------------------------------------------------------------------------- Family B
B_LENS = [0, 1, 63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256, 257, 718, 2047, 0, 0, 0, 2048, 2049, 4000, 5, 300, 1024, 1025, 0, 70,
          40, 500, 64, 900, 10, 0, 1100, 33, 1500, 700, 1300, 3, 600,              # the lengths of tests/test_gpu_composite_split.py
          1023, 1024, 1025, 4000, 718]
B_ZERO_RAY, B_DENSE_RAY = 14, 19
B_TAIL = {"tail2": [3, 70, 0, 128, 10, 513], "three": [7, 333, 0]}


def b_case(name="main", seed=921):
    key = ("B", name)
    if key in _cases:
        return _cases[key]
    lens = np.array(B_LENS if name == "main" else B_TAIL[name], np.int64)
    rng = np.random.default_rng(seed + len(lens))
    R = len(lens)
    offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    S = int(offs[-1])
    f32 = lambda a: a.astype(np.float32)
    color = f32(rng.uniform(0, 1, (S, 3)))
    dens = f32(rng.uniform(0, 30, (S, 1)) * (rng.uniform(size=(S, 1)) < 0.6))
    delt = rng.uniform(1e-3, 4e-2, (S, 1))
    for r in range(R):                                       # a total tau of 1 to 12: the transmittance survives to the ray's tail
        b, e = offs[r], offs[r + 1]
        tot = float((dens[b:e].astype(np.float64) * delt[b:e]).sum())
        if tot > 0:
            delt[b:e] *= rng.uniform(1.0, 12.0) / tot
    delt = f32(delt)
    if name == "main":
        assert lens[B_ZERO_RAY] == 718 and lens[B_DENSE_RAY] == 2048
        dens[offs[B_ZERO_RAY]:offs[B_ZERO_RAY + 1]] = 0.0
        dens[offs[B_DENSE_RAY]:offs[B_DENSE_RAY + 1]] = 30.0
        delt[offs[B_DENSE_RAY]:offs[B_DENSE_RAY + 1]] = 0.04
    c = dict(name=name, R=R, S=S, lens=lens, offs=offs, ray=np.repeat(np.arange(R), lens), color=color, density=dens, delta=delt,
             depths=f32(rng.uniform(1, 5, (S, 1))), g_rgb=f32(rng.normal(size=(R, 3))), g_alpha=f32(rng.normal(size=(R, 1))),
             g_depth=f32(rng.normal(size=(R, 1))), gt=f32(rng.uniform(-1.5, 2.5, (R, 3))), bg=BG_B)
    _cases[key] = c
    return c


def reference_b(c, g_rgb, g_alpha=None, g_depth=None, with_depths=True):
    """float64 per ray from the fp32 inputs:  w_i = T_i (1 - e_i), T_i = exp(-sum_{k<i} tau_k), e_i = exp(-tau_i);
    dL/dc_i = w_i g_rgb ; G_i = g_rgb.(c_i - bg) + g_alpha + g_depth t_i ; dL/dsigma_i = (G_i T_i e_i - sum_{k>i} G_k w_k) delta_i.
    -> (values, scale, scale_e).  scale: A_i = (|G|_i T_i e_i + sum over the WHOLE ray |G|_k w_k) delta_i (1 + total tau) for grad_density
    and its analogues.  scale_e adds what those leave out, the rounding of e_k = expf(-tau_k) in front of 1 - e_k: one unit in the last
    place of a value just below 1 is 2^-24 ABSOLUTE, so w_k carries 2^-24 T_k e_k however small 1 - e_k is, and a sum over the ray
    carries the sum of those (a faithfully rounded expf errs to one side, so they do not average out)."""
    R, S, offs = c["R"], c["S"], c["offs"]
    bg = np.array(np.float32(c["bg"]), np.float64)
    col, dn, dl, t = (c[k].astype(np.float64) for k in ("color", "density", "delta", "depths"))
    g_rgb = np.asarray(g_rgb, np.float64)
    ga = np.zeros((R, 1)) if g_alpha is None else np.asarray(g_alpha, np.float64)
    gdp = np.zeros((R, 1)) if (g_depth is None or not with_depths) else np.asarray(g_depth, np.float64)
    out = dict(rgb=np.zeros((R, 3)), alpha=np.zeros((R, 1)), depth=np.zeros((R, 1)), weights=np.zeros((S, 1)), grad_color=np.zeros((S, 3)),
               grad_density=np.zeros((S, 1)))
    scale = {k: np.zeros_like(v) for k, v in out.items()}
    extra = {k: np.zeros_like(v) for k, v in out.items()}
    for r in range(R):
        b, e = offs[r], offs[r + 1]
        tau = dn[b:e, 0] * dl[b:e, 0]
        excl = np.cumsum(tau) - tau
        T, et = np.exp(-excl), np.exp(-tau)
        w = T * (1.0 - et)
        tt = 1.0 + tau.sum()
        sa = w.sum()
        out["rgb"][r] = bg * (1.0 - sa) + (w[:, None] * col[b:e]).sum(0)
        out["alpha"][r], out["depth"][r] = sa, (w * t[b:e, 0]).sum()
        scale["rgb"][r] = tt * (w[:, None] * np.abs(col[b:e])).sum(0)
        scale["alpha"][r], scale["depth"][r] = tt * sa, tt * (w * np.abs(t[b:e, 0])).sum()
        G = (g_rgb[r] * (col[b:e] - bg)).sum(1) + ga[r, 0] + gdp[r, 0] * t[b:e, 0]
        aG = (np.abs(g_rgb[r]) * np.abs(col[b:e] - bg)).sum(1) + abs(ga[r, 0]) + np.abs(gdp[r, 0] * t[b:e, 0])
        gw = G * w
        suffix = gw[::-1].cumsum()[::-1] - gw
        out["weights"][b:e, 0], scale["weights"][b:e, 0] = w, tt * w
        out["grad_color"][b:e], scale["grad_color"][b:e] = w[:, None] * g_rgb[r], tt * w[:, None] * np.abs(g_rgb[r])
        out["grad_density"][b:e, 0] = (G * T * et - suffix) * dl[b:e, 0]
        scale["grad_density"][b:e, 0] = (aG * T * et + (aG * w).sum()) * dl[b:e, 0] * tt
        Te = T * et
        extra["rgb"][r] = (Te[:, None] * (np.abs(col[b:e]) + np.abs(bg))).sum(0)
        extra["alpha"][r], extra["depth"][r] = Te.sum(), (Te * np.abs(t[b:e, 0])).sum()
        extra["weights"][b:e, 0], extra["grad_color"][b:e] = Te, Te[:, None] * np.abs(g_rgb[r])
        extra["grad_density"][b:e, 0] = (aG * Te).sum() * dl[b:e, 0]
    out["hit"] = out["alpha"][:, 0] > 0
    return out, scale, {k: scale[k] + extra[k] for k in scale}


def reference_b_loss(c, kind):
    """wisp_composite_loss in float64: the forward, the trainer's loss, and the backward with g_rgb = d loss / d rgb"""
    fwd = reference_b(c, np.zeros((c["R"], 3)))[0]
    l, d = loss_terms(fwd["rgb"] - c["gt"].astype(np.float64), kind)
    out, scale, scale_e = reference_b(c, d / (3 * c["R"]))
    out["loss"] = l.mean()
    return out, scale, scale_e
