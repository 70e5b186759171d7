"""float64 restatement of the fused nglod field query and its central-difference gradient (csrc/sdf_eval.hip), and a generator of
exactly representable cases.  Test infrastructure only; host only (numpy + torch CPU), built on oracle/spc.py.

The field: an octree with feature tables on the corners of the active levels; per level the trilinear blend of the 8 corner rows
of the cell that holds the point ('sum' over the levels; zero where the point is outside [-1,1]^3 or the cell is unoccupied);
decoder W2 relu(W1 [position, features] + b1) + b2.  `half_round` rounds table entries and every level's blend through fp16, as
OctreeGrid.half_features does.

Exact cases (the technique of tests/spc_exact_ref.py / decoder_exact_ref.py): a point lies in cell `pt` of the finest level Lf at
offset k / 2^b per axis, so that c = (pt + k / 2^b) / 2^Lf * 2 - 1 is an fp32 value and the weights of a level d levels coarser are
multiples of 2^(-3 (b + d)); tables hold integers in [-1, 1], decoder weights -1 / 0 / 1, biases small integers.  Every product
and every partial sum, in any order, is then a multiple of one quantum with fewer than 2^24 quanta: exact in fp32 - a kernel must
equal the float64 result BIT FOR BIT whatever its summation order.  `check_exact` asserts those conditions: a failure there means
the inputs are bad, not that a kernel is wrong.  With a dyadic eps the six positions of the gradient are such points too (b grows
by the bits of eps), and (f+ - f-) / (2 eps) is exact.
"""
import numpy as np
import torch

from oracle import spc as ospc

F64 = np.float64


class Shell:
    """sparse octree: the cells of `level` whose centre lies in a spherical shell around the origin, with dual corners"""

    def __init__(self, level=4, r0=0.45, r1=0.8):
        n = 2 ** level
        g = np.stack(np.meshgrid(*[np.arange(n)] * 3, indexing='ij'), -1).reshape(-1, 3)
        r = np.linalg.norm((g + 0.5) / n * 2 - 1, axis=1)
        self.level = level
        self.cells = g[(r >= r0) & (r <= r1)]
        self.octree = ospc.points_to_octree(self.cells, level)
        self.points, self.pyramid, self.exsum = ospc.octree_to_spc(self.octree)
        self.points_dual, self.pyramid_dual = ospc.make_dual(self.points, self.pyramid)
        self.trinkets, self.parents = ospc.make_trinkets(self.points, self.pyramid, self.points_dual, self.pyramid_dual)
        occ = np.zeros((n, n, n), dtype=bool)
        occ[tuple(self.cells.T)] = True
        self.empty_cells = g[~occ.reshape(-1)]

    def rows(self, l):
        """rows of the feature table of level l as OctreeGrid allocates it (corners + 1)"""
        return int(self.pyramid_dual[0, l]) + 1

    def chain(self, coords32, levels):
        """[n, len(levels)] point index of the cell of every level (-1: none), by the fp32 rule of the octree query"""
        full = ospc.query(self.octree, self.exsum, np.asarray(coords32, dtype=np.float32), levels[-1], with_parents=True)
        return full[:, list(levels)]


_shells = {}


def shell(level=4):
    if level not in _shells:
        _shells[level] = Shell(level)
    return _shells[level]


# ---------------------------------------------------------------------------------------------------- the field in float64
def features(sh, fld, coords, dtype=torch.float64):
    """[n, 16] summed level blends at coords (f32 tensor [n, 3]) in `dtype`; also the chain"""
    levels = fld["levels"]
    c32 = coords.numpy().astype(np.float32)
    chain = sh.chain(c32, levels)
    c = coords.to(dtype)
    total = torch.zeros(c.shape[0], fld["feats"][0].shape[1], dtype=dtype)
    for li, l in enumerate(levels):
        p = chain[:, li]
        valid = p >= 0
        pts = torch.from_numpy(sh.points[np.where(valid, p, 0)].astype(F64)).to(dtype)
        f = float(2 ** l) * (0.5 * c + 0.5) - pts
        g = 1.0 - f
        w = torch.stack([(f if j & 4 else g)[:, 0] * (f if j & 2 else g)[:, 1] * (f if j & 1 else g)[:, 2] for j in range(8)], 1)
        table = fld["feats"][li].float()
        if fld["half_round"]:
            table = table.half()
        rows = torch.from_numpy(sh.trinkets[np.where(valid, p, 0)].astype(np.int64))
        acc = (w[:, :, None] * table.to(dtype)[rows]).sum(1)
        if fld["half_round"]:
            acc = acc.half().to(dtype)
        total = total + torch.where(torch.from_numpy(valid)[:, None], acc, torch.zeros_like(acc))
    return total, chain


def reference(sh, fld, coords, dtype=torch.float64):
    """raw decoder outputs [n, rows] at coords (f32 [n, 3]), evaluated in `dtype`"""
    feat, _ = features(sh, fld, coords, dtype)
    x = torch.cat([coords.to(dtype), feat], dim=1)
    h = torch.relu(x @ fld["w1"].to(dtype).T + fld["b1"].to(dtype))
    return h @ fld["w2"].to(dtype).reshape(-1, h.shape[1]).T + fld["b2"].to(dtype)


def offsets(coords, eps):
    """the six positions of the central difference, formed in fp32: [3, 2, n, 3] (axis, +/-)"""
    e = torch.eye(3) * np.float32(eps)
    return torch.stack([torch.stack([coords + e[a], coords - e[a]]) for a in range(3)])


def gradient_reference(sh, fld, coords, eps, dtype=torch.float64):
    """[n, 3] (f+ - f-) / (2 eps) on the last output row, all in `dtype` from the fp32 positions"""
    pos = offsets(coords, eps)
    cols = []
    for a in range(3):
        fp = reference(sh, fld, pos[a, 0], dtype)[:, -1]
        fm = reference(sh, fld, pos[a, 1], dtype)[:, -1]
        cols.append((fp - fm) / torch.tensor(2.0 * float(np.float32(eps)), dtype=dtype))
    return torch.stack(cols, 1)


# ---------------------------------------------------------------------------------------------------- exact cases
TREE_LEVEL = 4
OUTSIDE = np.array([[1.5, 0.25, -0.5], [-2.0, -2.0, 2.0], [0.0, 0.0, 1.25]])


def exact_points(sh, n, b=1, seed=0):
    """f32 [n, 3]: points of occupied cells at offsets k / 2^b (every 5th at k = 0: on the cell's faces, weights exactly 0 and
    1), every 7th in an EMPTY cell, every 11th outside the cube, and the cube's far corner (1, 1, 1)"""
    rng = np.random.default_rng(seed)
    Lf = sh.level
    cells = sh.cells[rng.integers(0, sh.cells.shape[0], size=n)].astype(F64)
    k = rng.integers(0, 2 ** b, size=(n, 3)).astype(F64)
    k[::5] = 0
    idx = np.arange(n)
    em = idx % 7 == 3
    cells[em] = sh.empty_cells[rng.integers(0, sh.empty_cells.shape[0], size=int(em.sum()))]
    c = (cells + k / 2.0 ** b) / 2.0 ** Lf * 2.0 - 1.0
    out = idx % 11 == 5
    c[out] = OUTSIDE[np.arange(int(out.sum())) % 3]
    if n > 2:
        c[2] = 1.0
    c32 = c.astype(np.float32)
    assert np.array_equal(c32.astype(F64), c)
    return torch.from_numpy(c32)


def exact_field(sh, levels, hidden, rows, seed=0, w2_nonzero=None, dtype=torch.float32, half_round=False):
    """tables of integers in [-1, 1] (table dtype `dtype`), W1 with three entries of -1 / 1 per row, b1 in [-1, 1], W2 of -1 / 1
    (w2_nonzero entries per row, all when None), b2 integers"""
    rng = np.random.default_rng(seed)
    feats = [torch.from_numpy(rng.integers(-1, 2, size=(sh.rows(l), 16)).astype(np.float32)).to(dtype) for l in levels]
    w1 = np.zeros((hidden, 19), dtype=np.float32)
    for h in range(hidden):
        cols = rng.choice(19, size=3, replace=False)
        w1[h, cols] = rng.choice([-1.0, 1.0], size=3)
    b1 = rng.integers(-1, 2, size=hidden).astype(np.float32)
    w2 = rng.choice([-1.0, 1.0], size=(rows, hidden)).astype(np.float32)
    if w2_nonzero is not None and w2_nonzero < hidden:
        for r in range(rows):
            w2[r, rng.permutation(hidden)[w2_nonzero:]] = 0.0
    b2 = rng.integers(-2, 3, size=rows).astype(np.float32)
    return dict(levels=tuple(int(l) for l in levels), feats=feats, half_round=bool(half_round), w1=torch.from_numpy(w1),
                b1=torch.from_numpy(b1), w2=torch.from_numpy(w2), b2=torch.from_numpy(b2))


def check_exact(sh, fld, coords, b):
    """assert the exactness conditions for the query at `coords` (points on the 2^-b sub-grid of the finest cells, or outside)"""
    levels = fld["levels"]
    q = 2.0 ** (-3 * (b + sh.level - levels[0]))                   # every weight, blend and input is a multiple of q
    q = min(q, 2.0 ** -(sh.level - 1 + b))                         # ... and so is every coordinate of the sub-grid
    feat, chain = features(sh, fld, coords)
    c = coords.double()
    x = torch.cat([c, feat], 1)
    assert bool(torch.equal(torch.round(x / q) * q, x)), "an input of the decoder is off the quantum grid"
    if fld["half_round"]:
        for li in range(len(levels)):
            one = dict(fld, levels=levels[li:li + 1], feats=fld["feats"][li:li + 1], half_round=False)
            blend = features(sh, one, coords)[0]
            assert bool(torch.equal(blend.half().double(), blend)), "a level blend is no fp16 value"
    w1, b1, w2, b2 = (fld[k].double() for k in ("w1", "b1", "w2", "b2"))
    s1 = x.abs() @ w1.abs().T + b1.abs()
    assert float(s1.max()) / q < 2.0 ** 24, "hidden layer: the partial sums leave fp32"
    h = torch.relu(x @ w1.T + b1)
    s2 = h @ w2.reshape(-1, h.shape[1]).abs().T + b2.abs()
    assert float(s2.max()) / q < 2.0 ** 24, "output layer: the partial sums leave fp32"
    return chain


def exact_case(levels=(2, 3, 4), hidden=128, rows=1, n=1000, b=1, seed=0, dtype=torch.float32, half_round=False,
               w2_nonzero=None):
    sh = shell(TREE_LEVEL)                                         # (levels may stop above the finest cells: a middle lod_idx)
    fld = exact_field(sh, levels, hidden, rows, seed=seed + 17 * hidden + rows, w2_nonzero=w2_nonzero, dtype=dtype,
                      half_round=half_round)
    coords = exact_points(sh, n, b=b, seed=seed + n)
    chain = check_exact(sh, fld, coords, b)
    return dict(shell=sh, field=fld, coords=coords, chain=chain, b=b)


GRAD_EPS = 2.0 ** -6          # the dyadic eps of the exact gradient cases


def exact_gradient_case(levels=(2, 3, 4), hidden=128, rows=1, n=1000, seed=0, dtype=torch.float32):
    """points on the half-cell sub-grid (b = 1) differenced with eps = 2^-6: the six positions lie on the 2^-3 sub-grid of the
    finest cells (b = 3).  Sixteen W2 entries per row keep the output sums inside 2^24 quanta; no fp16 rounding (a blend with
    15 fraction bits is no fp16 value)."""
    case = exact_case(levels, hidden, rows, n, b=1, seed=seed, dtype=dtype, half_round=False, w2_nonzero=16)
    sh, fld = case["shell"], case["field"]
    b_eps = 7 - sh.level                                            # 2^-6 = 2^(1 - Lf - b) at Lf = 4  ->  b = 3
    assert b_eps >= 1
    pos = offsets(case["coords"], GRAD_EPS)
    for a in range(3):
        for s in range(2):
            assert bool(torch.equal(pos[a, s].double(), case["coords"].double() + (1 - 2 * s) * GRAD_EPS * torch.eye(3)[a].double()))
            check_exact(sh, fld, pos[a, s], b_eps)
    case["eps"] = GRAD_EPS
    return case


# ---------------------------------------------------------------------------------------------------- generic cases
def generic_points(n, seed=0):
    """uniform in [-1.1, 1.1]^3 (some outside), every 9th snapped to a cell face of level 4, one at the origin (an empty cell)"""
    rng = np.random.default_rng(seed)
    c = rng.uniform(-1.1, 1.1, size=(n, 3)).astype(np.float32)
    c[::9, 0] = np.round(c[::9, 0] * 8) / 8
    c[0] = 0.0
    return torch.from_numpy(c)


def generic_field(sh, levels, hidden, rows, seed=0, dtype=torch.float32, half_round=True, std=0.05):
    g = torch.Generator().manual_seed(seed)
    feats = [(torch.randn(sh.rows(l), 16, generator=g) * std).to(dtype) for l in levels]
    k1, k2 = 1.0 / 19 ** 0.5, 1.0 / hidden ** 0.5

    def uni(shape, k):
        return (torch.rand(*shape, generator=g) * 2 - 1) * k
    return dict(levels=tuple(int(l) for l in levels), feats=feats, half_round=bool(half_round), w1=uni((hidden, 19), k1),
                b1=uni((hidden,), k1), w2=uni((rows, hidden), k2), b2=uni((rows,), k2))


def sphere_sdf(coords, radius=0.625):
    return coords.double().norm(dim=1).float() - radius
