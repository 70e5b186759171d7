"""float64 restatement of the fused triplanar SDF field (csrc/triplane_sdf_eval.hip) and its central-difference gradient, and a
generator of exactly representable cases.  Test infrastructure only; host only (numpy + torch CPU).

The field: NeuralSDF over a TriplanarGrid - per level and plane the source coordinates of wisp_reflect_source_index
(csrc/grid_sample_dev.h; restated here in fp32, operation by operation: the kernel forms them in fp32 and everything behind them is
evaluated in float64 FROM those fp32 values) for (y, z) on plane x, (x, z) on plane y, (x, y) on plane z; x0 = floor(ix), tx = ix -
x0, weights (1-tx)(1-ty), tx(1-ty), (1-tx)ty, tx ty, a corner with x0 + 1 >= size or y0 + 1 >= size left out; columns [x | y | z]
per level, 'cat' puts the levels behind one another, 'sum' adds them; decoder w2 . relu(W1 [position, features] + b1) + b2.  A
field is a dict: planes (list of 3 L f32 tensors [F, R_l, R_l]: x, y, z of level 0, then level 1, ...), multiscale 'cat' | 'sum',
w1 [hidden, 3 + K], b1 [hidden], w2 [hidden], b2 [1].

Exact cases: plane sizes 2^k + 1 for k in 2..5 and coordinates g = m / 2^(b + 4) - 1 for integers m, so that the source coordinate
ix = (m / 2^b) 2^(k - 5) is a dyadic number with b + 5 - k fraction bits on every level.  The reflection is exact as well (x / span
with a power-of-two span), so m also ranges over positions outside the cube, |g| <= 1.5.  Every `texel_every`-th point lies on a
texel line of every level (tx == 0), every 7th has a coordinate at g == 1 exactly (ix == span: the +1 corners fall outside the
plane), every 11th at g == -1.  Planes hold integers in [-1, 1], decoder weights -1 / 0 / 1, biases small integers: every product
and partial sum, in any order, is a multiple of one quantum 2^-bits (bits = 2 (b + 3): two blend factors of the coarsest level)
with fewer than 2^24 quanta - a kernel must equal the float64 result BIT FOR BIT.  `check_exact` asserts all of it: a failure there
blames the inputs, not the kernel.
"""
import numpy as np
import torch

F64 = np.float64
F32 = np.float32
EXACT_K = (2, 3, 4, 5)
EXACT_SIZES = tuple(2 ** k + 1 for k in EXACT_K)               # 5, 9, 17, 33


def source_index(g, size):
    """wisp_reflect_source_index in fp32, one rounding per operation: g f32 array -> f32 array in [0, size - 1]"""
    g = np.asarray(g, dtype=F32)
    span = F32(size - 1)
    if size <= 1:
        return np.zeros_like(g)
    x = np.abs((g + F32(1.0)) * F32(0.5) * span).astype(F32)
    flips = np.floor((x / span).astype(F32)).astype(F32)
    extra = (x - (flips * span).astype(F32)).astype(F32)
    odd = (np.minimum(flips, F32(2147483520.0)).astype(np.int64) & 1).astype(bool)
    x = np.where(odd, (span - extra).astype(F32), extra)
    return np.minimum(np.maximum(x, F32(0.0)), span).astype(F32)


def plane_lookup(plane, gx, gy, dtype=torch.float64):
    """[n, F]: bilinear lookup of plane [F, R, R] at grid_sample coordinates (gx -> width, gy -> height) in `dtype`"""
    R = int(plane.shape[-1])
    ix, iy = source_index(gx, R), source_index(gy, R)
    fx, fy = np.floor(ix), np.floor(iy)
    x0, y0 = torch.from_numpy(fx.astype(np.int64)), torch.from_numpy(fy.astype(np.int64))
    tx, ty = torch.from_numpy(ix - fx).to(dtype), torch.from_numpy(iy - fy).to(dtype)        # exact in fp32 (Sterbenz)
    p = plane.reshape(plane.shape[-3], R, R).to(dtype)
    out = torch.zeros(gx.shape[0], p.shape[0], dtype=dtype)
    for dy, dx, w in ((0, 0, (1 - tx) * (1 - ty)), (0, 1, tx * (1 - ty)), (1, 0, (1 - tx) * ty), (1, 1, tx * ty)):
        ok = (x0 + dx < R) & (y0 + dy < R)
        v = p[:, torch.clamp(y0 + dy, max=R - 1), torch.clamp(x0 + dx, max=R - 1)].T             # [n, F]
        out = out + torch.where(ok, w, torch.zeros_like(w))[:, None] * v
    return out


def num_lods(fld):
    return len(fld["planes"]) // 3


def plane_features(fld):
    return int(fld["planes"][0].shape[-3])


def num_cols(fld):
    return (1 if fld["multiscale"] == 'sum' else num_lods(fld)) * 3 * plane_features(fld)


def level_features(fld, coords, dtype=torch.float64):
    """[n, L, 3 F]: the [x | y | z] columns of every level"""
    c = coords.float().numpy()
    out = []
    for l in range(num_lods(fld)):
        px, py, pz = fld["planes"][3 * l:3 * l + 3]
        out.append(torch.cat([plane_lookup(px, c[:, 1], c[:, 2], dtype), plane_lookup(py, c[:, 0], c[:, 2], dtype),
                              plane_lookup(pz, c[:, 0], c[:, 1], dtype)], 1))
    return torch.stack(out, 1)


def features(fld, coords, dtype=torch.float64):
    """[n, K] what TriplanarGrid.interpolate returns at lod_idx = L - 1, in `dtype`"""
    lev = level_features(fld, coords, dtype)
    if fld["multiscale"] == 'cat':
        return lev.reshape(lev.shape[0], -1)
    acc = torch.zeros_like(lev[:, 0])
    for l in range(lev.shape[1]):                                                     # level order
        acc = acc + lev[:, l]
    return acc


def reference(fld, coords, dtype=torch.float64):
    """signed distance [n, 1] at coords (f32 [n, 3]), evaluated in `dtype`"""
    x = torch.cat([coords.to(dtype), features(fld, coords, dtype)], dim=1)
    h = torch.relu(x @ fld["w1"].to(dtype).T + fld["b1"].to(dtype))
    return h @ fld["w2"].to(dtype).reshape(1, -1).T + fld["b2"].to(dtype)


def offsets(coords, eps):
    """the six positions of the central difference, formed in fp32: [3, 2, n, 3] (axis, +/-)"""
    e = torch.eye(3) * np.float32(eps)
    return torch.stack([torch.stack([coords + e[a], coords - e[a]]) for a in range(3)])


def gradient_reference(fld, coords, eps, dtype=torch.float64):
    """[n, 3] (f+ - f-) / (2 eps), all in `dtype` from the fp32 positions"""
    pos = offsets(coords, eps)
    cols = []
    for a in range(3):
        fp = reference(fld, pos[a, 0], dtype)[:, 0]
        fm = reference(fld, pos[a, 1], dtype)[:, 0]
        cols.append((fp - fm) / torch.tensor(2.0 * float(np.float32(eps)), dtype=dtype))
    return torch.stack(cols, 1)


# ---------------------------------------------------------------------------------------------------- exact cases
def exact_points(n, b=1, margin=0, seed=0, texel_every=5):
    """f32 [n, 3]: g = m / 2^(b + 4) - 1 with integer m, |g| <= 1.5 - margin / 2^(b + 4); see the module docstring for the points
    on texel lines and on the faces"""
    rng = np.random.default_rng(seed)
    unit = 2 ** (b + 4)                                                             # m per unit of g
    lo, hi = -unit // 2 + margin, 2 * unit + unit // 2 - margin                  # g in [-1.5, 1.5]
    m = rng.integers(lo, hi + 1, size=(n, 3)).astype(F64)
    line = 2 ** b * 8                                                               # texel line of the coarsest level (k = 2)
    m[::texel_every] = unit + np.trunc((m[::texel_every] - unit) / line) * line      # (towards the centre: stays inside the range)
    pick = rng.integers(0, 3, size=n)
    rows = np.arange(n)
    m[rows[3::7], pick[3::7]] = 2 * unit                                            # g == 1
    m[rows[6::11], pick[6::11]] = 0                                                 # g == -1
    g = m / unit - 1.0
    g32 = g.astype(F32)
    assert np.array_equal(g32.astype(F64), g)
    return torch.from_numpy(g32)


def exact_field(hidden, F=4, multiscale='sum', sizes=EXACT_SIZES[-1:], seed=0, w2_nonzero=None):
    """planes of integers in [-1, 1], W1 with three entries of -1 / 1 per row, b1 in [-1, 1], w2 of -1 / 1 (w2_nonzero entries, all
    when None), b2 an integer"""
    rng = np.random.default_rng(seed)
    planes = [torch.from_numpy(rng.integers(-1, 2, size=(F, R, R)).astype(F32)) for R in sizes for _ in range(3)]
    K = (1 if multiscale == 'sum' else len(sizes)) * 3 * F
    w1 = np.zeros((hidden, 3 + K), dtype=F32)
    for h in range(hidden):
        cols = rng.choice(3 + K, size=3, replace=False)
        w1[h, cols] = rng.choice([-1.0, 1.0], size=3)
    b1 = rng.integers(-1, 2, size=hidden).astype(F32)
    w2 = rng.choice([-1.0, 1.0], size=hidden).astype(F32)
    if w2_nonzero is not None and w2_nonzero < hidden:
        w2[rng.permutation(hidden)[w2_nonzero:]] = 0.0
    b2 = rng.integers(-2, 3, size=1).astype(F32)
    return dict(planes=planes, multiscale=multiscale, w1=torch.from_numpy(w1), b1=torch.from_numpy(b1), w2=torch.from_numpy(w2),
                b2=torch.from_numpy(b2))


def exact_source_index(g64, size):
    """the source coordinate in exact (float64) arithmetic for dyadic g and a power-of-two span"""
    span = float(size - 1)
    if size <= 1:
        return np.zeros_like(g64)
    x = np.abs((g64 + 1.0) * 0.5 * span)
    flips = np.floor(x / span)
    extra = x - flips * span
    return np.clip(np.where(flips.astype(np.int64) & 1, span - extra, extra), 0.0, span)


def check_exact(fld, coords, bits):
    """assert the exactness conditions for the query at `coords`: on every level the fp32 source coordinate IS the exact one, every
    blend factor, feature and decoder input is a multiple of q = 2^-bits, every partial sum stays below 2^24 quanta"""
    q = 2.0 ** -bits
    c = coords.float().numpy()
    for l in range(num_lods(fld)):
        R = int(fld["planes"][3 * l].shape[-1])
        assert R == 1 or (R - 1) & (R - 2) == 0, "the span is no power of two: the reflection is not exact"
        ix = source_index(c, R)
        assert np.array_equal(ix.astype(F64), exact_source_index(c.astype(F64), R)), "a source coordinate is not exact in fp32"
        t = (ix - np.floor(ix)).astype(F64)
        assert np.array_equal(np.round(t / 2.0 ** -(bits // 2)) * 2.0 ** -(bits // 2), t), "a blend factor is off the quantum grid"
    for p in fld["planes"]:
        assert bool(torch.equal(torch.round(p), p)) and float(p.abs().max()) <= 1.0, "a plane holds more than -1 / 0 / 1"
    x = torch.cat([coords.double(), features(fld, coords)], 1)
    assert bool(torch.equal(torch.round(x / q) * q, x)), "an input of the decoder is off the quantum grid"
    lev = level_features(fld, coords).abs().sum(1)
    assert float(lev.max()) / q < 2.0 ** 24, "level sum: the partial sums leave fp32"
    w1, b1, w2, b2 = (fld[k].double() for k in ("w1", "b1", "w2", "b2"))
    for w in (w1, b1, w2, b2):
        assert bool(torch.equal(torch.round(w), w)), "a decoder parameter is no integer"
    s1 = x.abs() @ w1.abs().T + b1.abs()
    assert float(s1.max()) / q < 2.0 ** 24, "hidden layer: the partial sums leave fp32"
    h = torch.relu(x @ w1.T + b1)
    s2 = h @ w2.abs() + b2.abs()
    assert float(s2.max()) / q < 2.0 ** 24, "output layer: the partial sums leave fp32"


def _bits(b, sizes):
    """fraction bits of the quantum: two blend factors of the coarsest power-of-two level, or the coordinate itself (b + 4 bits)"""
    ks = [int(np.log2(R - 1)) for R in sizes if R > 1]
    return max(2 * max(b + 5 - min(ks), 0) if ks else 0, b + 4)


def exact_case(hidden=128, F=4, multiscale='sum', sizes=EXACT_SIZES[-1:], n=1000, seed=0, w2_nonzero=None, b=1):
    fld = exact_field(hidden, F, multiscale, sizes, seed=seed + 17 * hidden + F, w2_nonzero=w2_nonzero)
    coords = exact_points(n, b=b, seed=seed + n)
    bits = _bits(b, sizes)
    check_exact(fld, coords, bits)
    return dict(field=fld, coords=coords, bits=bits)


GRAD_EPS = 2.0 ** -6


def exact_gradient_case(hidden=128, F=4, multiscale='sum', sizes=EXACT_SIZES[-1:], n=1000, seed=0, b=1):
    """points on the b = 1 lattice differenced with eps = 2^-6: the six positions lie on the b = 2 lattice (one more fraction bit
    per blend factor), `margin` keeps them inside |g| <= 1.5.  Sixteen w2 entries keep the output sums small."""
    eps = GRAD_EPS
    b_pos = max(b, int(-np.log2(eps)) - 4)
    fld = exact_field(hidden, F, multiscale, sizes, seed=seed + 17 * hidden + F, w2_nonzero=16)
    coords = exact_points(n, b=b, margin=1, seed=seed + n)
    bits = _bits(b_pos, sizes)
    pos = offsets(coords, eps)
    for a in range(3):
        for s in range(2):
            assert bool(torch.equal(pos[a, s].double(), coords.double() + (1 - 2 * s) * eps * torch.eye(3)[a].double()))
            assert float(pos[a, s].abs().max()) <= 1.5
            check_exact(fld, pos[a, s], bits)
    return dict(field=fld, coords=coords, bits=bits, eps=eps)


# ---------------------------------------------------------------------------------------------------- generic cases
def generic_points(n, seed=0):
    """a third uniform inside the cube, a third with one or more coordinates exactly on c = +-1, a third outside (up to +-1.3:
    reflected by the grid); one at the origin"""
    rng = np.random.default_rng(seed)
    c = rng.uniform(-1.0, 1.0, size=(n, 3)).astype(F32)
    face = np.arange(n) % 3 == 1
    pick = rng.integers(0, 3, size=n)
    sign = rng.choice([-1.0, 1.0], size=n).astype(F32)
    c[face, pick[face]] = sign[face]
    out = np.arange(n) % 3 == 2
    c[out] = rng.uniform(-1.3, 1.3, size=(int(out.sum()), 3)).astype(F32)
    c[out, pick[out]] = sign[out] * rng.uniform(1.0, 1.3, size=int(out.sum())).astype(F32)
    c[0] = 0.0
    if n > 4:
        c[1], c[4] = 1.0, -1.0
    return torch.from_numpy(c)


def generic_field(sizes, hidden, F=4, multiscale='sum', seed=0, std=0.5):
    """random normal planes, nn.Linear initialisation (uniform +- 1 / sqrt(fan_in))"""
    g = torch.Generator().manual_seed(seed)
    planes = [torch.randn(F, R, R, generator=g) * std for R in sizes for _ in range(3)]
    K = (1 if multiscale == 'sum' else len(sizes)) * 3 * F
    k1, k2 = 1.0 / (3 + K) ** 0.5, 1.0 / hidden ** 0.5

    def uni(shape, k):
        return (torch.rand(*shape, generator=g) * 2 - 1) * k
    return dict(planes=planes, multiscale=multiscale, w1=uni((hidden, 3 + K), k1), b1=uni((hidden,), k1), w2=uni((hidden,), k2),
                b2=uni((1,), k2))


def sphere_sdf(coords, radius=0.55):
    return coords.double().norm(dim=1).float() - radius
