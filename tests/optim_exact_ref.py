"""Rounding-faithful references for the optimizer kernels (csrc/misc.hip: wisp_adamw_step, wisp_adamw_step_groups,
wisp_optim_step_groups) and for the AdamW step folded into the hash-grid reduce kernel's flush (csrc/hashgrid.hip).  Test
infrastructure only; host only (numpy + torch CPU).

AdamW (wisp_adamw_update, csrc/wisp_common.h) has no freedom: contraction is pinned, and mul, add, fma, sqrt and div are correctly
rounded, so `adamw_update` restates it in fp32 operation by operation and a kernel must equal it BIT FOR BIT.  numpy's float32
arithmetic is IEEE (denormals kept); the fma is exact: the float64 product of two fp32 values is exact (48 bits), TwoSum gives the
error of the float64 sum, the sum is nudged to the neighbour with an odd last bit when it was inexact (round to odd) and then
rounded once to fp32 - 53 bits are more than 24 + 2, so the double rounding is innocuous, for denormal results as well.  The bias
corrections call the C library's powf through ctypes, as the launchers do on the host: glibc's powf is not the correctly rounded
power.

Adam with L2 decay and RMSprop (kinds 1 and 2 of wisp_optim_step_groups) leave contraction to the compiler, so there is no single
bit pattern.  `bounded_groups` evaluates them in float64 and carries a running error bound per element: every fp32 operation adds
u = 2^-24 times the magnitude its result can have (|value| + bound so far), products and quotients add 2^-150 for a result in the
denormal range, and the bound is propagated through the following operations (product rule, quotient rule, the concavity of the
square root).  No other factor enters.  A contraction only removes a rounding, so the bound holds for every choice the compiler
can make.  (float64's own rounding, 2^-29 of one fp32 rounding per operation, is not modelled.)
"""
import ctypes
import ctypes.util
import math
from fractions import Fraction

import numpy as np
import torch

F32 = np.float32
F64 = np.float64
ONE = F32(1.0)
U = 2.0 ** -24                    # unit roundoff of fp32
TINY = 2.0 ** -150                # half the spacing of the fp32 denormals
MIN_NORMAL = 2.0 ** -126

_libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
_libm.powf.restype = ctypes.c_float
_libm.powf.argtypes = [ctypes.c_float, ctypes.c_float]


def powf(x, y):
    """the C library's powf on fp32 arguments -> np.float32"""
    return F32(_libm.powf(float(F32(x)), float(F32(y))))


def bias_corrections(beta1, beta2, step):
    """(1.0f - powf(beta1, (float)step), sqrtf(1.0f - powf(beta2, (float)step))) as the launchers form them on the host"""
    s = F32(step)
    return ONE - powf(beta1, s), np.sqrt(ONE - powf(beta2, s))


# ---------------------------------------------------------------------------------------------------- exact fma
def _f32(x):
    x = np.asarray(x)
    assert x.dtype == np.float32, x.dtype
    return x


def fma32(a, b, c):
    """fl32(a * b + c) with ONE rounding, elementwise over fp32 arrays or scalars"""
    shape = np.broadcast(a, b, c).shape
    a, b, c = (np.atleast_1d(_f32(x)).astype(F64) for x in (a, b, c))
    p = a * b                                     # exact: 24 + 24 bits, exponents far inside float64's
    s = p + c
    t = s - p                                     # TwoSum: s + e = p + c exactly
    e = (p - (s - t)) + (c - t)
    nudge = (e != 0) & ((s.view(np.int64) & 1) == 0)     # inexact and even: the other neighbour of the true sum is the odd one
    s = np.where(nudge, np.nextafter(s, np.where(e > 0, np.inf, -np.inf)), s)
    out = s.astype(F32)
    return out.reshape(shape) if shape else F32(out[0])


def fma32_twice_rounded(a, b, c):
    """what does NOT qualify: float64 product, float64 add, cast (two roundings)"""
    return (_f32(a).astype(F64) * _f32(b).astype(F64) + _f32(c).astype(F64)).astype(F32)


# ---------------------------------------------------------------------------------------------------- AdamW, bit for bit
MUTANTS = ("eps_in_sqrt", "coupled_decay", "bc2_no_sqrt", "unfused_moments", "flush_v", "recip_div")


def adamw_update(p, m, v, g, lr, wd, b1, b2, eps, bc1, bc2_sqrt, mutant=None):
    """wisp_adamw_update in fp32: every scalar and every operation rounded separately, the two moment updates and the parameter
    update single-rounded fmas.  g already carries the gradient scale.  -> (p, m, v).  `mutant` breaks it on purpose (host tests)."""
    p, m, v, g = _f32(p), _f32(m), _f32(v), _f32(g)
    lr, wd, b1, b2, eps, bc1, bc2_sqrt = (F32(x) for x in (lr, wd, b1, b2, eps, bc1, bc2_sqrt))
    assert mutant is None or mutant in MUTANTS, mutant
    if mutant == "coupled_decay":
        g = fma32(wd, p, g)
    else:
        p = p * (ONE - lr * wd)
    if mutant == "unfused_moments":
        m = b1 * m + (ONE - b1) * g
        v = b2 * v + ((ONE - b2) * g) * g
    else:
        m = fma32(b1, m, (ONE - b1) * g)
        v = fma32(b2, v, ((ONE - b2) * g) * g)
    if mutant == "flush_v":
        v = np.where(np.abs(v) < F32(MIN_NORMAL), F32(0.0), v)
    if mutant == "eps_in_sqrt":
        denom = np.sqrt(v + eps) / bc2_sqrt
    elif mutant == "bc2_no_sqrt":
        denom = np.sqrt(v) / (bc2_sqrt * bc2_sqrt) + eps
    elif mutant == "recip_div":
        denom = np.sqrt(v) * (ONE / bc2_sqrt) + eps
    else:
        denom = np.sqrt(v) / bc2_sqrt + eps
    q = m * (ONE / denom) if mutant == "recip_div" else m / denom
    p = fma32(-(lr / bc1), q, p)
    return p, m, v


def shadow_of(p, truncate=False):
    """the bf16 shadow: torch.bfloat16 round-to-nearest-even of the updated parameter (truncate: the mutant)"""
    p = np.ascontiguousarray(_f32(p))
    if truncate:
        p = (p.view(np.uint32) & np.uint32(0xFFFF0000)).view(np.float32)
    return torch.from_numpy(p.copy()).bfloat16()


def adamw_groups(p, m, v, g, groups, beta1, beta2, eps, step, grad_scale=1.0, zero_grad=False, mutant=None):
    """One launch of wisp_adamw_step_groups / wisp_optim_step_groups(kind 0) / the folded flush over whole buffers.
    groups: (begin, len, lr, wd, wants_shadow).  -> dict(p, m, v, g [whole buffers, copies], shadows [bf16 tensor or None per group])"""
    p, m, v, g = (np.array(_f32(x), copy=True) for x in (p, m, v, g))
    bc1, bc2_sqrt = bias_corrections(beta1, beta2, step)
    shadows = []
    for begin, n, lr, wd, sh in groups:
        s = slice(int(begin), int(begin) + int(n))
        gs = g[s] * F32(grad_scale)                                  # one fp32 product
        p[s], m[s], v[s] = adamw_update(p[s], m[s], v[s], gs, lr, wd, beta1, beta2, eps, bc1, bc2_sqrt, mutant)
        if zero_grad:
            g[s] = 0.0
        shadows.append(shadow_of(p[s]) if sh else None)
    return dict(p=p, m=m, v=v, g=g, shadows=shadows)


def adamw_step(p, m, v, g, lr, beta1, beta2, eps, wd, step, grad_scale=1.0, zero_grad=False, shadow=False, mutant=None):
    """One launch of wisp_adamw_step over whole buffers -> dict(p, m, v, g, shadow)"""
    out = adamw_groups(p, m, v, g, [(0, np.size(p), lr, wd, shadow)], beta1, beta2, eps, step, grad_scale, zero_grad, mutant)
    out["shadow"] = out.pop("shadows")[0]
    return out


# ---------------------------------------------------------------------------------------------------- the same in Fractions
def round32(x):
    """Fraction -> the nearest fp32 value (ties to even, denormals kept) as a Fraction"""
    x = Fraction(x)
    if x == 0:
        return x
    a = abs(x)
    e = a.numerator.bit_length() - a.denominator.bit_length()
    if Fraction(2) ** e > a:
        e -= 1
    assert Fraction(2) ** e <= a < Fraction(2) ** (e + 1)
    q = max(e - 23, -149)
    scaled = a / Fraction(2) ** q
    n = scaled.numerator // scaled.denominator
    r = scaled - n
    if r > Fraction(1, 2) or (r == Fraction(1, 2) and n & 1):
        n += 1
    out = n * Fraction(2) ** q
    assert out < Fraction(2) ** 128
    return out if x > 0 else -out


def sqrt32(x):
    """correctly rounded fp32 square root of a non-negative Fraction (never denormal: sqrt(2^-149) > 2^-75)"""
    x = Fraction(x)
    if x == 0:
        return x
    e = x.numerator.bit_length() - x.denominator.bit_length()
    if Fraction(2) ** e > x:
        e -= 1
    q = e // 2 - 23                                          # 2^(e // 2) <= sqrt(x) < 2^(e // 2 + 1)
    t = x / Fraction(4) ** (q - 30)                          # 30 guard bits
    ti = t.numerator // t.denominator
    i = math.isqrt(ti)
    exact = (i * i == ti) and t.denominator == 1
    n, rem, half = i >> 30, i & ((1 << 30) - 1), 1 << 29
    if rem > half or (rem == half and (not exact or n & 1)):
        n += 1
    return n * Fraction(2) ** q


def adamw_update_fraction(p, m, v, g, lr, wd, b1, b2, eps, bc1, bc2_sqrt):
    """adamw_update of ONE element with exact rationals and one explicit rounding per operation"""
    R = round32
    p, m, v, g, lr, wd, b1, b2, eps, bc1, bc2_sqrt = (Fraction(float(F32(x))) for x in (p, m, v, g, lr, wd, b1, b2, eps, bc1, bc2_sqrt))
    p = R(p * R(1 - R(lr * wd)))
    m = R(b1 * m + R(R(1 - b1) * g))
    v = R(b2 * v + R(R(R(1 - b2) * g) * g))
    denom = R(R(sqrt32(v) / bc2_sqrt) + eps)
    p = R(-R(lr / bc1) * R(m / denom) + p)
    return p, m, v


# ---------------------------------------------------------------------------------------------------- kinds 1 and 2: fp32 variants
KIND_CHOICES = {"adam": (3, 3, 3, 2), "rmsprop": (3, 3, 2, 2)}       # contraction choices per sum (rmsprop without momentum: the third is unused)
KIND_MUTANTS = ("eps_in_sqrt", "decoupled_decay", "bc2_no_sqrt")


def _sum2(a, b, c, d, choice):
    """a * b + c * d: 0 no fma, 1 fma(a, b, c * d), 2 fma(c, d, a * b)"""
    if choice == 0:
        return a * b + c * d
    return fma32(a, b, c * d) if choice == 1 else fma32(c, d, a * b)


def kind_update_f32(kind, p, s1, s2, g, lr, wd, h0, h1, eps, bc1, bc2_sqrt, gscale, choice=(0, 0, 0, 0), mutant=None):
    """optim_groups_kernel<1 or 2> in fp32 for ONE legal contraction `choice` of its sums -> (p, s1, s2); s1 None for RMSprop
    without momentum.  `mutant` changes the formula."""
    p, s2, g = _f32(p), _f32(s2), _f32(g)
    lr, wd, h0, h1, eps, bc1, bc2_sqrt, gscale = (F32(x) for x in (lr, wd, h0, h1, eps, bc1, bc2_sqrt, gscale))
    assert mutant is None or mutant in KIND_MUTANTS
    if mutant == "decoupled_decay":
        x = g * gscale
        p = p * (ONE - lr * wd)
    else:
        x = _sum2(g, gscale, wd, p, choice[0])
    if kind == "rmsprop":
        s2 = _sum2(h0, s2, (ONE - h0) * x, x, choice[1])
        avg = np.sqrt(s2 + eps) if mutant == "eps_in_sqrt" else np.sqrt(s2) + eps
        if h1 > 0:
            s1 = fma32(h1, _f32(s1), x / avg) if choice[2] else h1 * _f32(s1) + x / avg
            p = fma32(-lr, s1, p) if choice[3] else p - lr * s1
        else:
            p = fma32(-lr, x / avg, p) if choice[3] else p - lr * (x / avg)
        return p, s1, s2
    s1 = _sum2(h0, _f32(s1), ONE - h0, x, choice[1])
    s2 = _sum2(h1, s2, (ONE - h1) * x, x, choice[2])
    if mutant == "eps_in_sqrt":
        denom = np.sqrt(s2 + eps) / bc2_sqrt
    elif mutant == "bc2_no_sqrt":
        denom = np.sqrt(s2) / (bc2_sqrt * bc2_sqrt) + eps
    else:
        denom = np.sqrt(s2) / bc2_sqrt + eps
    c, q = lr / bc1, s1 / denom
    p = fma32(-c, q, p) if choice[3] else p - c * q
    return p, s1, s2


# ---------------------------------------------------------------------------------------------------- kinds 1 and 2: running bound
class Tracked:
    """float64 value(s) with a bound on |what fp32 computed - value|"""
    __slots__ = ("v", "e")

    def __init__(self, v, e=0.0):
        self.v = np.asarray(v, dtype=F64)
        self.e = np.asarray(e, dtype=F64) + np.zeros_like(self.v)


def _rounded(v, e, tiny):
    return Tracked(v, e + U * (np.abs(v) + e) + (TINY if tiny else 0.0))


def t_mul(a, b):
    return _rounded(a.v * b.v, np.abs(a.v) * b.e + np.abs(b.v) * a.e + a.e * b.e, True)


def t_add(a, b, sign=1.0):
    return _rounded(a.v + sign * b.v, a.e + b.e, False)         # (a sum in the denormal range is exact)


def t_div(a, b):
    assert np.all(np.abs(b.v) > b.e), "a divisor's bound reaches zero"
    v = a.v / b.v
    return _rounded(v, (a.e + np.abs(v) * b.e) / (np.abs(b.v) - b.e), True)


def t_sqrt(a):
    assert np.all(a.v >= 0)
    v = np.sqrt(a.v)
    e = np.maximum(np.sqrt(a.v + a.e) - v, v - np.sqrt(np.maximum(a.v - a.e, 0.0)))
    return _rounded(v, e, False)


def kind_update_bounded(kind, p, s1, s2, g, lr, wd, h0, h1, eps, bc1, bc2_sqrt, gscale):
    """optim_groups_kernel<1 or 2> in float64 with the running bound -> (p, s1, s2) as Tracked (s1 None without momentum).
    Inputs enter with bound 0: fp32 values for a kernel (bounded_groups rounds the scalars as the launcher's float arguments are;
    the state is what the kernel left); float64 values where the host test holds the formula against torch.optim."""
    T = lambda x: Tracked(np.asarray(x, dtype=F64))
    p, s2, g = T(p), T(s2), T(g)
    lr, wd, h0, h1, eps, bc1, bc2_sqrt, gscale = (T(x) for x in (lr, wd, h0, h1, eps, bc1, bc2_sqrt, gscale))
    one = Tracked(1.0)
    x = t_add(t_mul(g, gscale), t_mul(wd, p))
    if kind == "rmsprop":
        s2 = t_add(t_mul(h0, s2), t_mul(t_mul(t_add(one, h0, -1.0), x), x))
        avg = t_add(t_sqrt(s2), eps)
        if float(h1.v) > 0:
            s1 = t_add(t_mul(h1, T(s1)), t_div(x, avg))
            p = t_add(p, t_mul(lr, s1), -1.0)
        else:
            s1 = None
            p = t_add(p, t_mul(lr, t_div(x, avg)), -1.0)
        return p, s1, s2
    s1 = t_add(t_mul(h0, T(s1)), t_mul(t_add(one, h0, -1.0), x))
    s2 = t_add(t_mul(h1, s2), t_mul(t_mul(t_add(one, h1, -1.0), x), x))
    denom = t_add(t_div(t_sqrt(s2), bc2_sqrt), eps)
    p = t_add(p, t_mul(t_div(lr, bc1), t_div(s1, denom)), -1.0)
    return p, s1, s2


def kind_scalars(kind, h0, h1, step):
    """(bc1, bc2_sqrt) as wisp_optim_step_groups forms them"""
    return (ONE, ONE) if kind == "rmsprop" else bias_corrections(h0, h1, step)


def bounded_groups(kind, p, s1, s2, g, groups, h0, h1, eps, step, grad_scale=1.0, zero_grad=False):
    """One launch of wisp_optim_step_groups(kind 'adam' or 'rmsprop') over whole buffers.
    -> dict(p, s1, s2: (float64 value, bound) [bound 0 and the input value outside the groups]; g: fp32; inside: bool mask)"""
    bc1, bc2_sqrt = kind_scalars(kind, h0, h1, step)
    use_s1 = kind != "rmsprop" or F32(h1) > 0
    out = {k: [np.asarray(_f32(x), dtype=F64).copy(), np.zeros(np.size(x))] for k, x in (("p", p), ("s2", s2))}
    out["s1"] = [np.asarray(_f32(s1), dtype=F64).copy(), np.zeros(np.size(s1))] if s1 is not None else None
    gn = np.array(_f32(g), copy=True)
    inside = np.zeros(np.size(p), dtype=bool)
    for begin, n, lr, wd, _ in groups:
        s = slice(int(begin), int(begin) + int(n))
        tp, t1, t2 = kind_update_bounded(kind, p[s], s1[s] if use_s1 else None, s2[s], g[s],
                                         *(F32(x) for x in (lr, wd, h0, h1, eps, bc1, bc2_sqrt, grad_scale)))
        for k, t in (("p", tp), ("s2", t2)) + ((("s1", t1),) if use_s1 else ()):
            out[k][0][s], out[k][1][s] = t.v, t.e
        if zero_grad:
            gn[s] = 0.0
        inside[s] = True
    out["g"], out["inside"] = gn, inside
    return out


# ---------------------------------------------------------------------------------------------------- inputs
K_LO, K_HI = -82, 30
TIE_STRIDE, TIE_FIRST = 29, 11
REGIMES = ("fresh", "mid")


def _plant_ties(p, idx, decay, rng):
    """p[idx] such that fl32(p * decay) lies exactly between two bf16 values (low half 0x8000); -> the indices that took"""
    k = idx.size
    hi = (rng.integers(0, 2, size=k) << 15) | (rng.integers(118, 130, size=k) << 7) | rng.integers(0, 128, size=k)
    t = ((hi.astype(np.uint32) << np.uint32(16)) | np.uint32(0x8000)).view(np.float32)
    c = np.broadcast_to(np.asarray(decay, dtype=F32), p.shape)[idx] if np.ndim(decay) else F32(decay)
    lo = (t.astype(F64) / c).astype(F32)
    for _ in range(3):
        lo = np.nextafter(lo, F32(-np.inf))
    took = np.zeros(k, dtype=bool)
    for _ in range(7):                                               # the quotient and three neighbours on either side
        hit = (lo * c == t) & ~took
        p[idx[hit]] = lo[hit]
        took |= hit
        lo = np.nextafter(lo, F32(np.inf))
    return idx[took]


def inputs(n, seed, regime, decay=None):
    """p, m, v, g (fp32 numpy [n]).  g = normal x 2^k with k spread evenly over [-82, 30] (tiny gradients square into the denormals
    and, under 2^-75, to zero; eps = 1e-15 decides under 2^-50), exact +0 every 17th and -0 every 19th element.  regime 'fresh': m = v = 0 (step 1);
    'mid': m about 0.3 g, v about g^2 (which underflows with g), and every 23rd element a zero gradient over a live state.
    decay (fp32 scalar or [n], the launch's 1 - lr wd): every 29th element becomes a planted shadow tie - zero gradient and state,
    and a parameter whose decayed value lies exactly between two bf16 values."""
    assert regime in REGIMES
    rng = np.random.default_rng(seed)
    span = K_HI - K_LO + 1
    k = K_LO + (np.arange(n) * 37) % span          # (37 and 113 are coprime: every exponent, evenly; an element keeps its exponent
                                                   #  from seed to seed, so that a tiny gradient meets a tiny state in steps 2 and 3)
    g = (rng.standard_normal(n) * 2.0 ** k).astype(F32)
    g[3::17] = 0.0
    g[5::19] = -0.0
    p = (rng.standard_normal(n) * 2.0 ** rng.integers(-6, 3, size=n)).astype(F32)
    if regime == "fresh":
        m, v = np.zeros(n, F32), np.zeros(n, F32)
    else:
        m = (0.3 * g.astype(F64) * (1.0 + 0.1 * rng.standard_normal(n))).astype(F32)
        v = (g.astype(F64) ** 2 * rng.uniform(0.5, 1.5, size=n)).astype(F32)
        g[7::23] = 0.0
    ties = np.zeros(0, dtype=np.int64)
    if decay is not None:
        ties = _plant_ties(p, np.arange(TIE_FIRST, n, TIE_STRIDE), decay, rng)
        g[ties], m[ties], v[ties] = 0.0, 0.0, 0.0
    return dict(p=p, m=m, v=v, g=g, ties=ties, regime=regime, seed=seed, n=n)


SHARES = ("denormal_v", "v_zero_g_nonzero", "eps_decides", "eps_invisible", "unchanged", "decay_only", "shadow_ties")


def reaches(case):
    """Shares of the elements, from the restatement alone.  case: dict(p, m, v, g, lr, wd, beta1, beta2, eps, step, grad_scale).
    denormal_v, v_zero_g_nonzero (the scaled gradient is not zero, its square underflowed), eps_decides (sqrt(v) / bc2_sqrt < eps),
    eps_invisible (> 2^20 eps), unchanged (the parameter keeps its bits), decay_only (it moved, and only by weight decay),
    shadow_ties (the updated parameter lies exactly between two bf16 values)."""
    bc1, bc2_sqrt = bias_corrections(case["beta1"], case["beta2"], case["step"])
    gs = case["g"] * F32(case["grad_scale"])
    p1, m1, v1 = adamw_update(case["p"], case["m"], case["v"], gs, case["lr"], case["wd"], case["beta1"], case["beta2"], case["eps"],
                              bc1, bc2_sqrt)
    r = np.sqrt(v1) / bc2_sqrt
    eps = F32(case["eps"])
    decayed = case["p"] * (ONE - F32(case["lr"]) * F32(case["wd"]))
    share = lambda mask: float(np.mean(mask))
    return dict(denormal_v=share((v1 != 0) & (np.abs(v1) < F32(MIN_NORMAL))),
                v_zero_g_nonzero=share((v1 == 0) & (gs != 0)),
                eps_decides=share(r < eps),
                eps_invisible=share(r > F32(2.0 ** 20) * eps),
                unchanged=share(p1.view(np.uint32) == case["p"].view(np.uint32)),
                decay_only=share((p1 == decayed) & (p1 != case["p"])),
                shadow_ties=share((np.ascontiguousarray(p1).view(np.uint32) & np.uint32(0xFFFF)) == np.uint32(0x8000)))


# ---------------------------------------------------------------------------------------------------- what the GPU file runs
HYPER = {
    # nerf_hash.yaml's betas and eps; the grid's learning rate (1e-3 x grid_lr_weight) so that 1 - lr wd is not 1 in fp32
    "hash": dict(lr=0.5, beta1=0.9, beta2=0.999, eps=1e-15, wd=1e-6),
    "second wd0": dict(lr=1e-2, beta1=0.85, beta2=0.99, eps=1e-8, wd=0.0),
    "second wd1e-2": dict(lr=1e-2, beta1=0.85, beta2=0.99, eps=1e-8, wd=1e-2),
}
GRAD_SCALES = (1.0, 1.0 / 128.0, 2.0 ** -30)
SIZES = (1, 3, 4, 5, 1023, 1025, 65539)
WRAP_N = 4096 * 256 * 4 + 4 * 256 + 3          # the smallest buffer that takes the flat kernels' grid-stride loop twice and ends ragged
FRESH_STEPS = (1, 2, 3)
MID_STEPS = (1000, 30000)
GROUP_LR = (0.5, 1e-3, 1e-2, 0.1, 3e-2)
KIND_HYPER = {
    "adam": [dict(h0=0.9, h1=0.999, eps=1e-15, wd=1e-6), dict(h0=0.85, h1=0.99, eps=1e-8, wd=1e-2)],
    "rmsprop": [dict(h0=0.99, h1=0.0, eps=1e-8, wd=0.0), dict(h0=0.99, h1=0.9, eps=1e-8, wd=1e-2)],
}


def group_layout(n, count, residues, wds):
    """`count` groups of a buffer of n elements: group k begins at residues[k] mod 4, has a length that is no multiple of 4 and its
    own learning rate; gaps lie between the groups and the last group ends with the buffer.  Under 64 elements: one group.
    -> [(begin, len, lr, wd)]"""
    if n < 64:
        return [(0, n, GROUP_LR[0], wds[0])]
    seg = n // count
    out = []
    for k in range(count):
        b = k * seg
        b += (residues[k] - b) % 4
        ln = (seg * 3 // 4) | 1
        if k == count - 1:
            ln = n - b if (n - b) % 4 else n - b - 1
        assert b + ln <= n and ln % 4 != 0 and (not out or out[-1][0] + out[-1][1] < b)
        out.append((b, ln, GROUP_LR[k], wds[k % len(wds)]))
    return out


def wrap_layout(api_groups, wds):
    """the WRAP_N buffer for the group launches: the first group alone takes the grid-stride loop twice and ends in a ragged
    chunk; the others follow it behind gaps.  -> (buffer size, groups)"""
    out = [(0, WRAP_N, GROUP_LR[0], wds[0])]
    b = WRAP_N + 5
    residues = (0, 1, 2, 3, 2) if api_groups == 5 else (0, 0, 0, 0)
    for k in range(1, api_groups):
        b += (residues[k] - b) % 4
        out.append((b, 61 + 2 * k, GROUP_LR[k], wds[k % len(wds)]))
        b += 61 + 2 * k + 7
    return b + 9, out


def decay_of(n, groups):
    """fp32 1 - lr wd per element of a group launch (1 outside the groups)"""
    d = np.ones(n, dtype=F32)
    for begin, ln, lr, wd in groups:
        d[begin:begin + ln] = ONE - F32(lr) * F32(wd)
    return d


def seed_of(n, step):
    return 1000 + 7 * (n % 997) + step


def start_state(n, step, decay=None):
    """the state a run of the GPU file starts from: fresh before step 1, mid-training before a late step"""
    return inputs(n, seed_of(n, step), "fresh" if step == 1 else "mid", decay)


def step_gradient(n, step):
    """the gradient of steps 2 and 3 of a fresh run (step 1 takes the start state's)"""
    return inputs(n, seed_of(n, step) + 500, "fresh")["g"]


def adamw_update_f64(p, m, v, g, lr, wd, b1, b2, eps, step):
    """the AdamW formula in float64 (host test: against torch.optim.AdamW)"""
    p = p * (1.0 - lr * wd)
    m = b1 * m + (1.0 - b1) * g
    v = b2 * v + (1.0 - b2) * g * g
    return p - (lr / (1.0 - b1 ** step)) * (m / (np.sqrt(v) / np.sqrt(1.0 - b2 ** step) + eps)), m, v


# ---------------------------------------------------------------------------------------------------- the folded step
FOLDED_HYPER = dict(lr=0.5, beta1=0.9, beta2=0.999, eps=1e-15, weight_decay=1e-2)
FOLDED = {
    # case of hashgrid_exact_ref.py -> (power-of-two grad_scale, the paths its test is there for)
    "adam dense one owner f32 F2 2d n5000": (2.0 ** -7, ("dense_one_owner", "odd_start", "uncovered")),
    "adam hashed one owner f32 F2 2d n5000": (2.0 ** -70, ("hashed_one_owner", "uncovered")),
    "adam dead suffix bf16 F2 2d n5000": (2.0 ** -7, ("hashed_one_owner", "tail", "odd_start", "uncovered")),
    "dead suffix bf16 F2 n5000": (2.0 ** 4, ("tail", "uncovered")),
}
FOLDED_NOT_FUSED = ("dead suffix f32 F4 n5000", "merge f32 F8 2d one owner n6000")      # F = 4 and 8: no fold is compiled for them


def folded_paths(case):
    """what the folded launch of a hash-grid case reaches, from bin_geometry / reaches of hashgrid_exact_ref.py, and the rows per
    level it must report as covered: a live level whose buckets have one reduce workgroup is covered whole (its owned rows), a
    level behind zero_from_col is stepped by the tail workgroups (every row first_idx gives it), anything else is the caller's."""
    import hashgrid_exact_ref as H
    geo, first = H.bin_geometry(case), case["first_idx"]
    fused = case["F"] == 2 and "binned" in H.reaches(case)
    paths, covered = set(), []
    for l, g in enumerate(geo):
        if not fused:
            covered.append(0)
        elif not g["live"]:
            covered.append(int(first[l + 1] - first[l]))
            paths.add("tail")
        elif g["owners"] == 1:
            covered.append(g["rows"])
            paths.add(("dense_one_owner" if g["buckets"] >= 2 else "dense_one_bucket") if g["dense"] else "hashed_one_owner")
            if g["odd_start"]:
                paths.add("odd_start")
        else:
            covered.append(0)
            paths.add("uncovered")
    return paths, covered


def folded_groups(case, covered, hyper=FOLDED_HYPER):
    """the covered rows as groups of the flat table"""
    F, first = case["F"], case["first_idx"]
    return [(int(first[l]) * F, c * F, hyper["lr"], hyper["weight_decay"], True) for l, c in enumerate(covered) if c > 0]
