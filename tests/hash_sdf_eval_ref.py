"""float64 restatement of the fused hash-grid SDF field (csrc/hash_sdf_eval.hip) and its central-difference gradient, and a generator
of exactly representable cases.  Test infrastructure only; host only (numpy + torch CPU), built on oracle/hashgrid.py.

The field: NeuralSDF over a HashGrid - per level the cell, the eight corner rows and the blend factors of
oracle.hashgrid.corner_setup (dense or hashed indices, coordinates outside the cube clamped), the blend of the 8 rows rounded
through the table dtype; 'cat' keeps the level columns l * F + k with those at or above zero_from_col = lod_idx * F zeroed
(hash_grid.py:226-229), 'sum' adds the levels and rounds through the table dtype once; decoder w2 . relu(W1 [position, features] +
b1) + b2.  A field is a dict: table [rows, F] (table dtype), begin (int64 [L + 1]), resolutions, bitwidth, multiscale 'cat' | 'sum',
lod_idx, w1 [hidden, 3 + K], b1 [hidden], w2 [hidden], b2 [1].

Exact cases (the technique of tests/sdf_eval_ref.py): resolutions [4, 8, 16, 32] with tables of 2^10 rows - levels 4 and 8 are
dense, 16 and 32 hashed.  A point lies in cell `cell` of the finest level at offset k / 2^b per axis: c = (cell + k / 2^b) / 16 - 1
is an fp32 value, its scaled position on the level of resolution r is (cell + k / 2^b) * r / 32 - a dyadic number with
log2(32 / r) + b fraction bits - and the blend factors are multiples of 2^(-3 (3 + b)).  The clamp min(x, r - 1 - 1e-5) must not
bite, or the position stops being dyadic: on the COARSEST level that asks for (cell + 1) / 32 <= 3 / 4, i.e. cell <= 23 - inside the
cell <= res_finest - 2 = 30 that keeps the finest level clear, and what MAX_CELL is.  (Below the cube the clamp max(x, 0) gives
exactly 0, which is harmless; the gradient cases keep `margin` cells away from MAX_CELL so that c + eps stays clear too.)  Tables
hold integers in [-1, 1], decoder weights -1 / 0 / 1, biases small integers: every product and partial sum, in any order, is a
multiple of one quantum with fewer than 2^24 quanta - a kernel must equal the float64 result BIT FOR BIT.  With a half table dtype
a level blend must be a value of that dtype as well: `step` keeps the cells on a coarser sub-grid (fewer fraction bits on the coarse
levels) - step 1, b = 0 for f16 (9 bits), step 4, b = 0 for bf16 (3 bits).  `check_exact` asserts all of it: a failure there blames
the inputs, not the kernel.
"""
import numpy as np
import torch

from oracle import hashgrid as ohg

F64 = np.float64
EXACT_RES = (4, 8, 16, 32)
EXACT_BITWIDTH = 10
MAX_CELL = 23


def level_blends(fld, coords, dtype=torch.float64):
    """[n, L, F] blend of every level at coords (f32 [n, 3]) in `dtype`, rounded through the table dtype"""
    table = fld["table"]
    T = 2 ** fld["bitwidth"]
    c32 = coords.float()
    out = []
    for l, res in enumerate(fld["resolutions"]):
        _, idx = ohg.corner_setup(c32, int(res), T)
        # the blend factors again, in `dtype`, from the fp32 position the kernel forms (one rounding of the exact value)
        x = ((c32.double() * 0.5 + 0.5) * float(res)).float()
        x = torch.clamp(x, min=0.0, max=float(np.float32(res - 1 - 1e-5)))
        f = (x - torch.floor(x)).to(dtype)
        g = 1.0 - f
        w = torch.stack([(f if j & 4 else g)[:, 0] * (f if j & 2 else g)[:, 1] * (f if j & 1 else g)[:, 2] for j in range(8)], 1)
        rows = table[int(fld["begin"][l]) + idx].to(dtype)                       # [n, 8, F]
        acc = (w[:, :, None] * rows).sum(1)
        if table.dtype != torch.float32:
            acc = acc.to(table.dtype).to(dtype)
        out.append(acc)
    return torch.stack(out, 1)


def features(fld, coords, dtype=torch.float64):
    """[n, K] what HashGrid.interpolate returns at lod_idx, in `dtype`"""
    lev = level_blends(fld, coords, dtype)
    n, L, F = lev.shape
    if fld["multiscale"] == 'cat':
        flat = lev.reshape(n, L * F).clone()
        flat[:, fld["lod_idx"] * F:] = 0
        return flat
    s = lev.sum(1)
    return s.to(fld["table"].dtype).to(dtype) if fld["table"].dtype != torch.float32 else s


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


def num_cols(fld):
    F = fld["table"].shape[1]
    return len(fld["resolutions"]) * F if fld["multiscale"] == 'cat' else F


def zero_from_col(fld):
    F = fld["table"].shape[1]
    return (fld["lod_idx"] if fld["multiscale"] == 'cat' else len(fld["resolutions"])) * F


# ---------------------------------------------------------------------------------------------------- exact cases
def exact_points(n, b=1, step=1, margin=0, seed=0):
    """f32 [n, 3]: c = (cell + k / 2^b) / 16 - 1 with cell a multiple of `step` in [0, MAX_CELL - margin]; every 5th point at
    k = 0 (on a cell face: blend factors exactly 0 and 1)"""
    rng = np.random.default_rng(seed)
    top = (MAX_CELL - margin) // step
    cell = (rng.integers(0, top + 1, size=(n, 3)) * step).astype(F64)
    k = rng.integers(0, 2 ** b, size=(n, 3)).astype(F64)
    k[::5] = 0
    c = (cell + k / 2.0 ** b) / 16.0 - 1.0
    c32 = c.astype(np.float32)
    assert np.array_equal(c32.astype(F64), c)
    return torch.from_numpy(c32)


def exact_field(hidden, F=8, multiscale='cat', lod_idx=3, dtype=torch.float32, seed=0, w2_nonzero=None):
    """table of integers in [-1, 1], W1 with three entries of -1 / 1 per row, b1 in [-1, 1], w2 of -1 / 1 (w2_nonzero entries, all
    when None), b2 an integer"""
    rng = np.random.default_rng(seed)
    _, begin = ohg.table_layout(EXACT_RES, 2 ** EXACT_BITWIDTH)
    table = torch.from_numpy(rng.integers(-1, 2, size=(int(begin[-1]), F)).astype(np.float32)).to(dtype)
    K = len(EXACT_RES) * F if multiscale == 'cat' else F
    w1 = np.zeros((hidden, 3 + K), dtype=np.float32)
    for h in range(hidden):
        cols = rng.choice(3 + K, size=3, replace=False)
        w1[h, cols] = rng.choice([-1.0, 1.0], size=3)
    b1 = rng.integers(-1, 2, size=hidden).astype(np.float32)
    w2 = rng.choice([-1.0, 1.0], size=hidden).astype(np.float32)
    if w2_nonzero is not None and w2_nonzero < hidden:
        w2[rng.permutation(hidden)[w2_nonzero:]] = 0.0
    b2 = rng.integers(-2, 3, size=1).astype(np.float32)
    return dict(table=table, begin=torch.from_numpy(begin), resolutions=list(EXACT_RES), bitwidth=EXACT_BITWIDTH,
                multiscale=multiscale, lod_idx=int(lod_idx), w1=torch.from_numpy(w1), b1=torch.from_numpy(b1),
                w2=torch.from_numpy(w2), b2=torch.from_numpy(b2))


def check_exact(fld, coords, bits):
    """assert the exactness conditions for the query at `coords`: every blend factor, level blend and decoder input is a multiple
    of q = 2^-bits, every partial sum stays below 2^24 quanta, and a level blend is a value of a half table dtype"""
    q = 2.0 ** -bits
    T = 2 ** fld["bitwidth"]
    for res in fld["resolutions"]:
        x64 = (coords.double() * 0.5 + 0.5) * float(res)
        assert float(x64.max()) < res - 1 - 1e-4, "the clamp bites: the scaled position is not dyadic"
        coef, _ = ohg.corner_setup(coords.float(), int(res), T)
        assert bool(torch.equal(torch.round(coef.double() / q) * q, coef.double())), "a blend factor is off the quantum grid"
    lev = level_blends(dict(fld, table=fld["table"].float()), coords)
    assert bool(torch.equal(torch.round(lev / q) * q, lev)), "a level blend is off the quantum grid"
    td = fld["table"].dtype
    if td != torch.float32:
        assert bool(torch.equal(lev.to(td).double(), lev)), f"a level blend is no {td} value"
        if fld["multiscale"] == 'sum':
            s = lev.sum(1)
            assert bool(torch.equal(s.to(td).double(), s)), f"a level sum is no {td} value"
    x = torch.cat([coords.double(), features(fld, coords)], 1)
    assert bool(torch.equal(torch.round(x / q) * q, x)), "an input of the decoder is off the quantum grid"
    w1, b1, w2, b2 = (fld[k].double() for k in ("w1", "b1", "w2", "b2"))
    s1 = x.abs() @ w1.abs().T + b1.abs()
    assert float(s1.max()) / q < 2.0 ** 24, "hidden layer: the partial sums leave fp32"
    h = torch.relu(x @ w1.T + b1)
    s2 = h @ w2.abs() + b2.abs()
    assert float(s2.max()) / q < 2.0 ** 24, "output layer: the partial sums leave fp32"


# sub-grid of the exact points per table dtype: (b, step) -> 3 (3 + b - log2 step) fraction bits on the coarsest level
EXACT_GRID = {torch.float32: (1, 1), torch.float16: (0, 1), torch.bfloat16: (0, 4)}


def _bits(b, step):
    """fraction bits of the quantum: three blend factors of the coarsest level, or the coordinate itself (b + 4 bits)"""
    return max(3 * max(3 + b - int(np.log2(step)), 0), b + 4)


def exact_case(hidden=128, F=8, multiscale='cat', lod_idx=3, n=1000, seed=0, dtype=torch.float32, w2_nonzero=None):
    b, step = EXACT_GRID[dtype]
    fld = exact_field(hidden, F, multiscale, lod_idx, dtype, seed=seed + 17 * hidden + F, w2_nonzero=w2_nonzero)
    coords = exact_points(n, b=b, step=step, seed=seed + n)
    bits = _bits(b, step)
    check_exact(fld, coords, bits)
    return dict(field=fld, coords=coords, bits=bits)


# the dyadic eps of the exact gradient cases per table dtype, in finest cells of 1 / 16: the six positions stay on a sub-grid whose
# level blends are values of the table dtype
GRAD_EPS = {torch.float32: 2.0 ** -6, torch.float16: 2.0 ** -4, torch.bfloat16: 2.0 ** -2}


def exact_gradient_case(hidden=128, F=8, multiscale='cat', lod_idx=3, n=1000, seed=0, dtype=torch.float32):
    """f32 tables: points on the half-cell sub-grid (b = 1) differenced with eps = 2^-6 - the six positions lie on the 2^-2
    sub-grid of the finest cells (15 fraction bits on the coarsest level).  f16 / bf16: eps is one / four finest cells, so the
    positions stay on the sub-grid of the query case.  Sixteen w2 entries keep the output sums inside 2^24 quanta."""
    b, step = EXACT_GRID[dtype]
    eps = GRAD_EPS[dtype]
    margin = max(int(np.ceil(eps * 16)), 1)
    fld = exact_field(hidden, F, multiscale, lod_idx, dtype, seed=seed + 17 * hidden + F, w2_nonzero=16)
    coords = exact_points(n, b=b, step=step, margin=margin, seed=seed + n)
    b_pos = max(b, int(-np.log2(eps)) - 4)
    bits = _bits(b_pos, step)
    pos = offsets(coords, eps)
    for a in range(3):
        for s in range(2):
            assert bool(torch.equal(pos[a, s].double(), coords.double() + (1 - 2 * s) * eps * torch.eye(3)[a].double()))
            check_exact(fld, pos[a, s], bits)
    return dict(field=fld, coords=coords, bits=bits, eps=eps)


# ---------------------------------------------------------------------------------------------------- generic cases
GENERIC_RES = ([4, 9, 18, 40], [16, 80, 406, 2048])
GENERIC_BITWIDTH = 12


def generic_points(n, seed=0):
    """a third uniform inside the cube, a third with one or more coordinates exactly on c = +-1, a third outside (up to +-1.3:
    clamped by the grid); one at the origin"""
    rng = np.random.default_rng(seed)
    c = rng.uniform(-1.0, 1.0, size=(n, 3)).astype(np.float32)
    face = np.arange(n) % 3 == 1
    pick = rng.integers(0, 3, size=n)
    sign = rng.choice([-1.0, 1.0], size=n).astype(np.float32)
    c[face, pick[face]] = sign[face]
    out = np.arange(n) % 3 == 2
    c[out] = rng.uniform(-1.3, 1.3, size=(int(out.sum()), 3)).astype(np.float32)
    c[out, pick[out]] = sign[out] * rng.uniform(1.0, 1.3, size=int(out.sum())).astype(np.float32)
    c[0] = 0.0
    if n > 4:
        c[1], c[4] = 1.0, -1.0
    return torch.from_numpy(c)


def generic_field(resolutions, hidden, F=8, multiscale='cat', lod_idx=None, seed=0, dtype=torch.float32, std=0.05,
                  bitwidth=GENERIC_BITWIDTH):
    """random normal table, nn.Linear initialisation (uniform +- 1 / sqrt(fan_in))"""
    g = torch.Generator().manual_seed(seed)
    _, begin = ohg.table_layout(resolutions, 2 ** bitwidth)
    table = (torch.randn(int(begin[-1]), F, generator=g) * std).to(dtype)
    L = len(resolutions)
    K = L * F if multiscale == 'cat' else F
    k1, k2 = 1.0 / (3 + K) ** 0.5, 1.0 / hidden ** 0.5

    def uni(shape, k):
        return (torch.rand(*shape, generator=g) * 2 - 1) * k
    return dict(table=table, begin=torch.from_numpy(begin), resolutions=[int(r) for r in resolutions], bitwidth=bitwidth,
                multiscale=multiscale, lod_idx=L - 1 if lod_idx is None else int(lod_idx), w1=uni((hidden, 3 + K), k1),
                b1=uni((hidden,), k1), w2=uni((hidden,), k2), b2=uni((1,), k2))


def sphere_sdf(coords, radius=0.625):
    return coords.double().norm(dim=1).float() - radius
