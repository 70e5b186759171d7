"""Exact-arithmetic inputs and a plain float64 reference for the trilinear lookups of OctreeGrid / CodebookOctreeGrid and their
order-free backward (csrc/spc_interp.hip, csrc/spc_grad.hip).  Test infrastructure only; host only (numpy + torch CPU).

The technique (as tests/decoder_exact_ref.py): choose inputs for which EVERY product and EVERY partial sum is exactly
representable.  A sample lies in cell `pt` of the finest active level Lf at offset k / 2^b per axis, k in 0 .. 2^b - 1:
    c = (pt + k / 2^b) / 2^Lf * 2 - 1
is an fp32 value, `0.5 c + 0.5`, the scaling by 2^level and the subtraction of the cell origin are exact at every level, and
the eight weights of a level d levels coarser are multiples of 2^(-3 (b + d)).  Upstream gradients are small integers (times
one power of two), feature tables small integers.  Then a gradient does not depend on the order of the adds, on the run merge,
the corner links, the atomics or the binary point of the fixed-point accumulators, and a kernel must equal the float64
scatter-add below BIT FOR BIT.

`reference` / `codebook_reference` apply no rounding emulation and ASSERT the exactness conditions themselves: a failing assertion
here means the inputs are bad, not that a kernel is wrong.

SAMPLE ORDER is the subject.  The orderings lay runs of samples of one cell end to end without padding, so that runs start at
arbitrary lanes; `report` restates which samples the merge kernel of spc_grad.hip treats as run tails (128 samples per block, 64
per wave, segmented scan inside 16-lane rows) and says per level what a case reaches.
"""
import types

import numpy as np
import torch

from oracle import spc as ospc

F64 = np.float64
WAVE, ROW, BLOCK = 64, 16, 128
LINK_TAILS = 8                                    # SG_LINK_TAILS of spc_grad.hip: a wave with MORE tails links corners across tails
RUNS_MIXED = (1, 2, 15, 16, 17, 31, 33, 63, 64, 65, 129, 200)
RUNS_LONG = (20, 33, 64, 47, 129, 25, 70, 21)     # >= 20: at most 4 run ends + 4 row ends in any 64 lanes
LEVELS4 = (2, 3, 4, 5)


# ---------------------------------------------------------------------------------------------------- the tree
class Tree:
    """octree of `n` random points at `level` (the recipe of gpu_helpers._sparse_blas) with its dual corners; `extra`: further
    cells [m, 3] of `level` that the octree holds as well"""

    def __init__(self, level=5, n=3000, seed=401, extra=None):
        rng = np.random.default_rng(seed)
        P = rng.integers(0, 2 ** level, size=(n, 3))
        if extra is not None:
            P = np.concatenate([P, np.asarray(extra, dtype=P.dtype).reshape(-1, 3)])
        self.level, self.n, self.seed = level, n, seed
        self.octree = ospc.points_to_octree(P, level)
        self.points, self.pyramid, self.exsum = ospc.octree_to_spc(self.octree)
        self.points_dual, self.pyramid_dual = ospc.make_dual(self.points, self.pyramid)
        self.trinkets, self.parents = ospc.make_trinkets(self.points, self.pyramid, self.points_dual, self.pyramid_dual)
        self.morton = [ospc.points_to_morton(self.level_points(l)) for l in range(level + 1)]
        assert all(bool((np.diff(m) > 0).all()) for m in self.morton)

    def first(self, l):
        return int(self.pyramid[1, l])

    def count(self, l):
        return int(self.pyramid[0, l])

    def rows(self, l):
        return int(self.pyramid_dual[0, l])

    def level_points(self, l):
        return self.points[self.first(l):self.first(l) + self.count(l)].astype(np.int64)

    def lookup(self, l, xyz):
        """global point index of cell xyz [N, 3] of level l, -1 where the cell is empty or outside the grid"""
        xyz = np.asarray(xyz, dtype=np.int64)
        ok = ((xyz >= 0) & (xyz < 2 ** l)).all(1)
        m = ospc.points_to_morton(np.where(ok[:, None], xyz, 0))
        i = np.minimum(np.searchsorted(self.morton[l], m), self.count(l) - 1)
        return np.where(ok & (self.morton[l][i] == m), self.first(l) + i, -1)

    def oracle_blas(self):
        return types.SimpleNamespace(octree=self.octree, exsum=self.exsum, points=self.points, pyramid=self.pyramid)


# ---------------------------------------------------------------------------------------------------- sample orders
OUTSIDE = -1                                      # cell marker of a miss: the coordinate (2, 2, 2), outside every cell


def _lay_runs(cells_of_run, run_lengths, n):
    out = []
    r = 0
    while len(out) < n:
        out += [r] * run_lengths[r % len(run_lengths)]
        r += 1
    run = np.asarray(out[:n])
    return cells_of_run(run), run


def order_runs(tree, level, n, run_lengths, seed, misses=False):
    """cells [n, 3] of `level`: runs of the given lengths, laid end to end, every run in another occupied cell.  misses: every
    second run of three or more samples has a coordinate outside every cell in its middle; every fourth has a sample of the
    cell's EMPTY sibling there (no cell at `level`, the run's cells at the coarser levels), and so has every fifth sample-of-one."""
    rng = np.random.default_rng(seed)
    pts = tree.level_points(level)
    # (runs of four Morton neighbours follow each other: siblings, so that the runs of the coarser levels are longer)
    perm = (rng.permutation(pts.shape[0] // 4)[:, None] * 4 + np.arange(4)[None, :]).reshape(-1)
    cells, run = _lay_runs(lambda r: pts[perm[r % perm.shape[0]]], run_lengths, n)
    if misses:
        cells = cells.copy()
        sib = pts ^ np.array([1, 0, 0])
        empty = sib[tree.lookup(level, sib) < 0]
        starts = np.flatnonzero(np.diff(np.concatenate([[-1], run])) != 0)
        ends = np.concatenate([starts[1:], [n]])
        singles = 0
        for r, (s, e) in enumerate(zip(starts, ends)):
            if e - s >= 3 and r % 2 == 1:
                cells[s + (e - s) // 2] = OUTSIDE
            elif e - s >= 3 and r % 4 == 2:
                other = cells[s] ^ np.array([1, 0, 0])                 # the run's own sibling: the coarser levels' runs go on
                if tree.lookup(level, other[None])[0] < 0:
                    cells[s + (e - s) // 2] = other
            elif e - s == 1:
                if singles % 5 == 4:
                    cells[s] = empty[(r * 7) % empty.shape[0]]
                singles += 1
    return cells


def order_walk(tree, level, paths, path_len, passes, seed):
    """ray-like: `paths` walks through face-sharing occupied neighbour cells, each walked `passes` times (back and forth) with 1
    to 3 samples per cell visit - consecutive run tails share the four corner rows of a face."""
    rng = np.random.default_rng(seed)
    pts = tree.level_points(level)
    steps = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]])
    out = []
    used = set()
    for _ in range(paths):
        path = None
        for _try in range(200):
            cur = pts[rng.integers(0, pts.shape[0])]
            if tuple(cur) in used:
                continue
            path = [cur]
            while len(path) < path_len:
                nb = path[-1][None] + steps[rng.permutation(6)]
                nb = [c for c, p in zip(nb, tree.lookup(level, nb)) if p >= 0 and tuple(c) not in used
                      and not any((c == q).all() for q in path)]
                if not nb:
                    break
                path.append(nb[0])
            if len(path) >= 3:
                break
        assert path is not None and len(path) >= 3, "no walk of three face-sharing cells found"
        used.update(tuple(c) for c in path)
        for k in range(passes):
            for c in (path if k % 2 == 0 else path[::-1]):
                out += [c] * int(rng.integers(1, 4))
    return np.asarray(out, dtype=np.int64)


def regroup(tree, level, cells):
    """the permutation that brings all samples of a cell together (cells in Morton order): the long-run order of the same multiset"""
    key = np.where(cells[:, 0] >= 0, ospc.points_to_morton(np.maximum(cells, 0)), -1)
    return np.argsort(key, kind="stable")


# ---------------------------------------------------------------------------------------------------- what the merge kernel sees
def report(tree, chain):
    """Per chain column: the run tails spc_grad_scatter_merge_kernel finds, restated from its statements (key = cell or a per-lane
    dummy; tail = valid and (last lane of a 16-lane row or the next lane has another key); lane 63 has no next lane).
    Returns a list of dicts: tails_per_wave [waves], cross_row / cross_wave / cross_block (a run continues across a 16-lane
    boundary inside a wave / across lane 63 inside a block / across a multiple of 128), miss_inside (a miss between two samples
    of one cell), shared4 / shared8 (consecutive tails of a wave with more than LINK_TAILS tails that share 4 / 8 corner rows)."""
    chain = np.asarray(chain)
    N = chain.shape[0]
    Np = max(-(-N // WAVE) * WAVE, WAVE)
    idx = np.arange(Np)
    lane = idx % WAVE
    out = []
    for li in range(chain.shape[1]):
        p = np.full(Np, -1, dtype=np.int64)
        p[:N] = chain[:, li]
        key = np.where(p >= 0, p, -1 - lane)
        nxt = np.roll(key, -1)
        nxt[lane == WAVE - 1] = key[lane == WAVE - 1]
        tail = (p >= 0) & ((lane % ROW == ROW - 1) | (nxt != key))
        ntails = tail.reshape(-1, WAVE).sum(1)
        same_prev = np.zeros(Np, dtype=bool)
        same_prev[1:] = (p[1:] >= 0) & (p[1:] == p[:-1])
        shared4 = shared8 = 0
        for w in np.flatnonzero(ntails > LINK_TAILS):
            t = p[w * WAVE:(w + 1) * WAVE][tail[w * WAVE:(w + 1) * WAVE]]
            rows = tree.trinkets[t]
            common = (rows[:-1, :, None] == rows[1:, None, :]).any(2).sum(1)
            shared4 += int((common == 4).sum())
            shared8 += int((common == 8).sum())
        out.append(dict(tails_per_wave=ntails,
                        cross_row=int((same_prev & (idx % ROW == 0) & (idx % WAVE != 0)).sum()),
                        cross_wave=int((same_prev & (idx % WAVE == 0) & (idx % BLOCK != 0)).sum()),
                        cross_block=int((same_prev & (idx % BLOCK == 0)).sum()),
                        miss_inside=int(((p[1:-1] < 0) & (p[:-2] >= 0) & (p[:-2] == p[2:])).sum()),
                        shared4=shared4, shared8=shared8))
    return out


# ---------------------------------------------------------------------------------------------------- cases
def _ints(shape, lo, hi, rng):
    return rng.integers(lo, hi + 1, size=shape).astype(F64)


def make_case(tree, cells, levels, channels, sum_lods, b=1, seed=0, grad="ints", scale_exp=0, spv=1, pidx_holes=0):
    """One exact case on the CPU.  cells [N, 3]: the sample's cell at levels[-1] (OUTSIDE = a miss).  grad: 'ints' (integers in
    [-2, 2]), 'mix' (those, every 7th row / 2^3 and every 7th + 3 row * 2^2), 'unit' ([-1, 1]), 'huge' ({0, +-1}); all times
    2^scale_exp.  spv > 1: the Kaolin-style leaf layout - cells [V, 3], spv samples per voxel, coords [V, spv, 3], one level;
    pidx_holes: every pidx_holes-th voxel gets pidx = -1 although its coordinates lie in a cell."""
    rng = np.random.default_rng(seed)
    levels = tuple(int(l) for l in levels)
    Lf, L = levels[-1], len(levels)
    assert spv == 1 or L == 1
    cells = np.repeat(np.asarray(cells, dtype=np.int64), spv, axis=0)
    N = cells.shape[0]
    miss = cells[:, 0] < 0
    k = rng.integers(0, 2 ** b, size=(N, 3))
    k[::5] = 0                                                    # offset 0: weights of exactly 1 and 0
    c64 = np.where(miss[:, None], 2.0, (cells + k / 2.0 ** b) / 2.0 ** Lf * 2.0 - 1.0)
    coords = c64.astype(np.float32)
    assert np.array_equal(coords.astype(F64), c64), "inputs are not exact: a coordinate is not an fp32 value"
    chain = np.full((N, L), -1, dtype=np.int64)
    for li, l in enumerate(levels):
        chain[:, li] = np.where(miss, -1, tree.lookup(l, np.maximum(cells, 0) >> (Lf - l)))
    if pidx_holes:
        chain[(np.arange(N) // spv) % pidx_holes == 0] = -1
    width = channels if sum_lods else L * channels
    if grad == "huge":
        g = _ints((N, width), -1, 1, rng) * (rng.integers(0, 3, size=(N, 1)) == 0)      # most rows zero: few adds per table row
    elif grad == "unit":
        g = _ints((N, width), -1, 1, rng)
    else:
        g = _ints((N, width), -2, 2, rng)
    gq_exp = 0
    if grad == "mix":
        g[::7] *= 2.0 ** -3
        g[3::7] *= 2.0 ** 2
        gq_exp = -3
    g = g * 2.0 ** scale_exp
    g32 = g.astype(np.float32)
    assert np.array_equal(g32.astype(F64), g), "inputs are not exact: a gradient is not an fp32 value"
    feats = [_ints((tree.rows(l), channels), -2, 2, rng) for l in levels]
    seeds = [((np.arange(tree.rows(l) * channels).reshape(tree.rows(l), channels) * 7 + l) % 11 - 5).astype(F64) for l in levels]
    return dict(tree=tree, levels=levels, channels=channels, sum=bool(sum_lods), b=b, spv=spv, N=N,
                coords=torch.from_numpy(coords), chain=torch.from_numpy(chain), grad_out=torch.from_numpy(g32),
                feats=[torch.from_numpy(f.astype(np.float32)) for f in feats],
                seeds=[torch.from_numpy(s.astype(np.float32)) for s in seeds], quantum_exp=scale_exp + gq_exp,
                seeded=scale_exp == 0)            # (a scaled gradient is added to zeros: integer seeds + 2^-130 is no fp32 value)


def permuted(case, perm):
    """the same multiset of samples in another order (spv == 1)"""
    assert case["spv"] == 1
    perm = torch.as_tensor(perm)
    out = dict(case)
    for name in ("coords", "chain", "grad_out"):
        out[name] = case[name][perm].contiguous()
    return out


def truncated(case, n):
    """the first n samples of a case"""
    assert case["spv"] == 1
    out = dict(case)
    for name in ("coords", "chain", "grad_out"):
        out[name] = case[name][:n].contiguous()
    out["N"] = n
    return out


def weights(case, li):
    """[N, 8] float64 weights of chain column li (rows of misses hold the weights of point 0; callers mask them), corner j =
    dx << 2 | dy << 1 | dz.  Asserts that the kernel's fp32 statements (sg_coeffs / trilinear_coeffs) are exact on them."""
    tree, l = case["tree"], case["levels"][li]
    p = case["chain"][:, li].numpy()
    valid = p >= 0
    pts = tree.points[np.where(valid, p, 0)]
    c32 = case["coords"].numpy()
    f32 = np.float32(2 ** l) * (np.float32(0.5) * c32 + np.float32(0.5)) - pts.astype(np.float32)
    f = 2.0 ** l * (0.5 * c32.astype(F64) + 0.5) - pts.astype(F64)
    assert np.array_equal(f32[valid].astype(F64), f[valid]), "inputs are not exact: an in-cell position rounds in fp32"
    assert bool(((f[valid] >= 0) & (f[valid] < 1)).all()), "a sample lies outside the cell its chain names"
    g32, g = np.float32(1.0) - f32, 1.0 - f
    w = np.stack([(f if j & 4 else g)[:, 0] * (f if j & 2 else g)[:, 1] * (f if j & 1 else g)[:, 2] for j in range(8)], 1)
    w32 = np.stack([((f32 if j & 4 else g32)[:, 0] * (f32 if j & 2 else g32)[:, 1]) * (f32 if j & 1 else g32)[:, 2] for j in range(8)], 1)
    assert np.array_equal(w32[valid].astype(F64), w[valid]), "inputs are not exact: a weight rounds in fp32"
    q = 2.0 ** (-3 * (case["b"] + case["levels"][-1] - l))
    assert np.array_equal(np.round(w[valid] / q) * q, w[valid]), "a weight is off the level's grid"
    return w, valid


def _f32_exact(t):
    return bool(torch.equal(t.float().double(), t))


def reference(case, tables=None, check=True):
    """float64: per level the scatter-add of w_j * g into row trinkets[pidx, j] (the gradient of the level's table) and the forward
    lookup out = sum_j w_j table[trinkets[pidx, j]] ('sum' adds the levels, 'cat' puts them side by side).
    Returns dict(grads [L x f64 [rows, C]], abs_sums (same, of |w g|), touched [L x bool [rows]], out f64 [N, C or L C],
    out_levels [L x f64 [N, C]], half_ok: every per-level result and every table entry is an fp16 value)."""
    tree, levels, C = case["tree"], case["levels"], case["channels"]
    g_all = case["grad_out"].double()
    tables = [f.double() for f in (case["feats"] if tables is None else tables)]
    grads, abs_sums, touched, outs = [], [], [], []
    half_ok = True
    for li, l in enumerate(levels):
        w, valid = weights(case, li)
        w = torch.from_numpy(w[valid])
        rows = torch.from_numpy(tree.trinkets[case["chain"][:, li].numpy()[valid]].astype(np.int64))       # [Nv, 8]
        g = (g_all if case["sum"] else g_all[:, li * C:(li + 1) * C])[torch.from_numpy(valid)]
        contrib = w[:, :, None] * g[:, None, :]                                                           # [Nv, 8, C]
        grad = torch.zeros(tree.rows(l), C, dtype=torch.float64).index_add_(0, rows.reshape(-1), contrib.reshape(-1, C))
        asum = torch.zeros(tree.rows(l), C, dtype=torch.float64).index_add_(0, rows.reshape(-1), contrib.abs().reshape(-1, C))
        tch = torch.zeros(tree.rows(l), dtype=torch.bool)
        tch[rows.reshape(-1)] = True
        out = torch.zeros(case["N"], C, dtype=torch.float64)
        out[torch.from_numpy(valid)] = (w[:, :, None] * tables[li][rows]).sum(1)
        if check:
            q = 2.0 ** (case["quantum_exp"] - 3 * (case["b"] + levels[-1] - l))
            assert _f32_exact(contrib), f"inputs are not exact: a product w g of level {l} is not an fp32 value"
            assert bool(torch.equal(torch.round(contrib / q) * q, contrib)), f"level {l}: a product is off the grid of spacing {q}"
            # every partial sum, in any order, is a multiple of q below 2^24 q: exact in fp32
            assert float(asum.max()) / q < 2.0 ** 24, f"inputs are not exact: sum |w g| = {float(asum.max()) / q} quanta at level {l}"
            assert _f32_exact(grad) and (not case["seeded"] or _f32_exact(grad + case["seeds"][li].double())), f"level {l}: a gradient is not an fp32 value"
            assert _f32_exact(out), f"level {l}: a forward value is not an fp32 value"
        half_ok = half_ok and bool(torch.equal(out.half().double(), out)) and bool(torch.equal(tables[li].half().double(), tables[li]))
        grads.append(grad); abs_sums.append(asum); touched.append(tch); outs.append(out)
    total = sum(outs) if case["sum"] else torch.cat(outs, 1)
    if check:
        assert _f32_exact(total)
    return dict(grads=grads, abs_sums=abs_sums, touched=touched, out=total, out_levels=outs, half_ok=half_ok)


def max_adds_per_row(case):
    """the largest number of samples with a non-zero gradient that name one table row (for the nearly-overflowing case)"""
    tree, C = case["tree"], case["channels"]
    worst = 0
    for li, l in enumerate(case["levels"]):
        p = case["chain"][:, li].numpy()
        g = case["grad_out"] if case["sum"] else case["grad_out"][:, li * C:(li + 1) * C]
        live = (p >= 0) & (g != 0).any(1).numpy()
        worst = max(worst, int(np.bincount(tree.trinkets[p[live]].reshape(-1), minlength=1).max()))
    return worst


def thin_to(case, limit):
    """zero the gradient of samples, in order, that would give some table row more than `limit` non-zero contributions"""
    tree, C = case["tree"], case["channels"]
    g = case["grad_out"].clone()
    counts = [np.zeros(tree.rows(l), dtype=np.int64) for l in case["levels"]]
    chain = case["chain"].numpy()
    for i in np.flatnonzero((g != 0).any(1).numpy()):
        rows = [tree.trinkets[chain[i, li]] for li in range(len(case["levels"])) if chain[i, li] >= 0]
        live = [li for li in range(len(case["levels"])) if chain[i, li] >= 0]
        if any((counts[li][r] >= limit).any() for li, r in zip(live, rows)):
            g[i] = 0.0
        else:
            for li, r in zip(live, rows):
                counts[li][r] += 1
    out = dict(case)
    out["grad_out"] = g
    return out


# ---------------------------------------------------------------------------------------------------- codebook
def make_codebook(case, K, mode, seed=0):
    """logits [rows, K] and dictionaries [K, F] (F = case channels) that make the softmax exact.
    one-hot: key (5 r + 3 + level) mod K has logit 0, the others <= -200: expf underflows to exactly 0, p is exactly one-hot,
    the straight-through scale (1 - p) + p is exactly 1.  uniform: every logit 0.25, K a power of two: p = 1 / K exactly, and
    the first index wins the tie (key 0)."""
    assert mode in ("onehot", "uniform") and K & (K - 1) == 0
    tree, F = case["tree"], case["channels"]
    logits, dicts, keys, seeds_l, seeds_d = [], [], [], [], []
    for l in case["levels"]:
        R = tree.rows(l)
        r = np.arange(R)
        if mode == "onehot":
            key = (5 * r + 3 + l) % K
            lg = -200.0 - ((r[:, None] + np.arange(K)[None, :]) % 7).astype(F64)
            lg[r, key] = 0.0
        else:
            key = np.zeros(R, dtype=np.int64)
            lg = np.full((R, K), 0.25)
        D = ((np.arange(K)[:, None] * 3 + np.arange(F)[None, :] * 5 + l + seed + (np.arange(K)[:, None] // 3)) % 3 - 1).astype(F64)
        logits.append(torch.from_numpy(lg.astype(np.float32))); dicts.append(torch.from_numpy(D.astype(np.float32)))
        keys.append(torch.from_numpy(key))
        seeds_l.append(torch.from_numpy((((np.arange(R * K).reshape(R, K) * 5 + l) % 7) - 3).astype(np.float32)))
        seeds_d.append(torch.from_numpy((((np.arange(K * F).reshape(K, F) * 3 + l) % 5) - 2).astype(np.float32)))
    return dict(K=K, mode=mode, logits=logits, dicts=dicts, keys=keys, seeds_logits=seeds_l, seeds_dict=seeds_d)


def codebook_tables(cb):
    """the feature every logits row decodes to, training or evaluation: dictionary[key] (scale exactly 1)"""
    return [D[k] for D, k in zip(cb["dicts"], cb["keys"])]


def codebook_reference(case, cb, check=True):
    """float64 gradients of logits and dictionaries from G = the gradient of the decoded rows (reference(...)['grads']):
    one-hot: d logits = 0, d dictionary[key] = sum of the G of the rows with that key.
    uniform: d logits[r, k] = (D_k . G_r - mean_m D_m . G_r) / K, the whole G goes to dictionary row 0."""
    ref = reference(case, tables=codebook_tables(cb), check=check)
    K = cb["K"]
    g_logits, g_dicts = [], []
    for li, l in enumerate(case["levels"]):
        G, D = ref["grads"][li], cb["dicts"][li].double()
        q = 2.0 ** (case["quantum_exp"] - 3 * (case["b"] + case["levels"][-1] - l))
        gd = torch.zeros_like(D).index_add_(0, cb["keys"][li], G)
        gd_abs = torch.zeros_like(D).index_add_(0, cb["keys"][li], G.abs())
        if cb["mode"] == "onehot":
            gl = torch.zeros(G.shape[0], K, dtype=torch.float64)
        else:
            dk = G @ D.T
            mean = dk.sum(1, keepdim=True) / K
            gl = (dk - mean) / K
            if check:
                assert _f32_exact(dk) and _f32_exact(mean) and _f32_exact(dk - mean) and _f32_exact(gl), \
                    f"inputs are not exact: D . G, its mean or the quotient of level {l} is not an fp32 value"
                # the kernel adds the K terms p_k D_k . G one after the other: multiples of q / K, partial sums below 2^24 of them
                assert float(dk.abs().sum(1).max()) / q < 2.0 ** 24, f"level {l}: sum_k |D_k . G| / K reaches 2^24 quanta"
        if check:
            assert float(G.abs().sum(1).max()) / q < 2.0 ** 24
            assert float(gd_abs.max()) / q < 2.0 ** 24, f"inputs are not exact: a dictionary row of level {l} sums {float(gd_abs.max()) / q} quanta"
            assert _f32_exact(gd) and _f32_exact(gd + cb["seeds_dict"][li].double()) and _f32_exact(gl + cb["seeds_logits"][li].double())
        g_logits.append(gl); g_dicts.append(gd)
    ref["grad_logits"], ref["grad_dicts"] = g_logits, g_dicts
    return ref


# ---------------------------------------------------------------------------------------------------- the case families
TREE_SEED = 401
N_MAIN = 3000
N_SPLIT_BIG = 16500                # 16 channels: 16 n >= 256 * 1024, one lane group walks all levels of a sample
SMALL_N = (1, 63, 64, 65, 127, 128, 129)
MERGE_CHANNELS = (1, 2, 3, 4, 6, 7, 8)
WIDE_CHANNELS = (9, 12, 16, 33, 64, 72)
LOSS_SCALES = (16, 24, -30, -130)
HUGE_EXP = 121
HUGE_ADDS = 32

_trees = {}


def tree(seed=TREE_SEED):
    if seed not in _trees:
        _trees[seed] = Tree(5, 3000, seed)
    return _trees[seed]


def cells_of(order, n=N_MAIN, level=5):
    """the sample orders of the GPU file: 'mixed' (RUNS_MIXED with misses inside), 'few' (long runs: at most LINK_TAILS tails per
    wave), 'many' (ray-like walks: more), 'many_regrouped' (the samples of 'many', those of a cell together)"""
    t = tree()
    if order == "mixed":
        return order_runs(t, level, n, RUNS_MIXED, 11, misses=True)
    if order == "few":
        return order_runs(t, level, n, RUNS_LONG, 12)
    assert order == "many"
    return order_walk(t, level, paths=24, path_len=6, passes=22, seed=13)


def multi_case(order, channels, sum_lods, levels=LEVELS4, n=N_MAIN, grad="ints", scale_exp=0):
    cells = cells_of(order, n, levels[-1])
    return make_case(tree(), cells, levels, channels, sum_lods, b=1, seed=1000 + channels + 7 * len(levels) + (n % 997),
                     grad=grad, scale_exp=scale_exp)


def huge_case(channels):
    """|g| in {0, 2^121}: M >= 2^121 selects the float-atomic path with FINITE values; at most HUGE_ADDS non-zero contributions
    per table row, so that no sum reaches 2^127 (asserted)"""
    case = thin_to(multi_case("mixed", channels, True, grad="huge", scale_exp=HUGE_EXP), HUGE_ADDS)
    assert max_adds_per_row(case) <= HUGE_ADDS
    ref = reference(case)
    assert max(float(a.max()) for a in ref["abs_sums"]) < 2.0 ** 127
    return case


def leaf_case(level, S, channels, holes=17, n_voxels=None, seed=0):
    """Kaolin-style leaf call: coords [V, S, 3] inside voxels pidx [V] of one level, offsets k / 8; runs of voxels in one cell;
    every `holes`-th voxel has pidx -1"""
    V = n_voxels or max(2400 // S, 300)
    cells = order_runs(tree(), level, V, (1, 2, 3, 5, 9, 1, 17), 21 + S + seed)
    return make_case(tree(), cells, (level,), channels, True, b=3, seed=2000 + S + channels + level, spv=S, pidx_holes=holes)


def codebook_case(mode, K, F, sum_lods, levels=LEVELS4):
    """one-hot: the mixed order with integer gradients; uniform: half as many samples and gradients in {-1, 0, 1}, which keeps
    D . G, its mean over the keys and the quotient by K inside fp32 (asserted by codebook_reference)"""
    if mode == "onehot":
        case = multi_case("mixed", F, sum_lods, levels)
    else:
        case = multi_case("mixed", F, sum_lods, levels, n=N_MAIN // 2, grad="unit")
    return case, make_codebook(case, K, mode, seed=K + F)


def codebook_leaf_case(mode, K, F, level, S, n_voxels):
    case = leaf_case(level, S, F, n_voxels=n_voxels, seed=K)
    if mode == "uniform":
        case["grad_out"] = case["grad_out"].clamp(-1, 1)
    return case, make_codebook(case, K, mode, seed=K + F + 1)


def cancel_case(channels, sum_lods=True):
    """1024 long-run samples, the same samples again with the negated gradient, then 515 others: every table row that only the
    first two groups touch receives contributions that cancel to exactly zero (its accumulator returns to 0 and it keeps its seed)"""
    a = multi_case("few", channels, sum_lods, n=1024)
    b = multi_case("mixed", channels, sum_lods, n=515)
    out = dict(a)
    out["coords"] = torch.cat([a["coords"], a["coords"], b["coords"]])
    out["chain"] = torch.cat([a["chain"], a["chain"], b["chain"]])
    out["grad_out"] = torch.cat([a["grad_out"], -a["grad_out"], b["grad_out"]])
    out["N"] = 2 * a["N"] + b["N"]
    return out


def cancelled_rows(ref):
    """per level: rows that received non-zero contributions whose sum is exactly zero in every channel"""
    return [(a.sum(1) > 0) & (g == 0).all(1) for a, g in zip(ref["abs_sums"], ref["grads"])]
