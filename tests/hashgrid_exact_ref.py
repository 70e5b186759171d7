"""Exact-arithmetic inputs and a plain float64 reference for the hash-grid lookup, its backward, grad_coords and the corner query's
backward (csrc/hashgrid.hip, csrc/hashgrid_dev.h).  Test infrastructure only; host only (numpy + torch CPU).

The technique (as tests/decoder_exact_ref.py and tests/spc_exact_ref.py): choose inputs for which EVERY product and EVERY partial
sum is exactly representable.  Resolutions are powers of two (they may repeat); a sample lies in cell p of the finest resolution
Rf at offset k / 2^b per axis,
    c = (p + k / 2^b) / Rf * 2 - 1,
which is an fp32 value; res / 2 * c + res / 2 is exact at every level and the 2^dim blend factors of a level d octaves coarser are
multiples of u = 2^(-dim (b + d)).  Upstream gradients, table values and seeded outputs are small integers times one power of two.
Then a gradient depends neither on the order of the adds nor on the run merge, the buckets, the slots, the record form, the
binary point of the 64-bit fixed-point accumulators or the float atomics of the fallbacks, and a kernel must equal the float64
scatter-add below BIT FOR BIT.

The clamp bound fl32(res - 1 - 1e-5) is not dyadic below res 258: samples stay strictly below res - 1 on such levels.  From 258
on it rounds to res - 1 exactly, every coordinate is allowed, and c = +1 gives corner index `res` with a weight of exactly 0: the
spill row (the forward reads the next level's row, pinned to the table's last row on the last level; the backward drops a row
past the table).

Indices and weights come from oracle.hashgrid.corner_setup: the hash is not restated here.  The `reference_*` functions ASSERT the
exactness conditions themselves: a failing assertion here means the inputs are bad, not that a kernel is wrong.
"""
import numpy as np
import torch

from oracle import hashgrid as ohash

F64 = np.float64
RUNS = (1, 2, 3, 15, 16, 17, 33, 64, 65)
TILE = 64                                   # samples a wave merges over (HG_TILE; every emitter piece is a multiple of it)
DTYPES = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}
ZERO_CAP = 0.15                             # share of the elements with a non-zero weight that may end at exactly 0, per level


# ---------------------------------------------------------------------------------------------------- layout
def layout(res, bitwidth, dim, pad=None):
    """-> (rows owned per level [L], first_idx [L + 1] int64).  pad[l] unused rows in front of level l (a first_idx whose end fits
    the table is all the package asks for)."""
    sizes, begin = ohash.table_layout(res, 2 ** bitwidth, dim)
    if pad is not None:
        begin = begin.copy()
        shift = 0
        for l in range(len(res)):
            shift += int(pad[l])
            begin[l] += shift
        begin[len(res)] += shift
    return sizes, begin


def bin_geometry(case):
    """Per level what bin_plan of hashgrid.hip derives from the public sizes: dense, rows owned, bucket entries (the largest
    power of two <= 16384 / F), buckets, owners per bucket (min(64 // buckets, emitting pieces), at least 1) for pieces of 1024
    samples, whether the level starts on an odd row, and whether a sample names a row past the rows the level owns."""
    F, dim, T = case["F"], case["dim"], 2 ** case["bitwidth"]
    centries = 1 << int(np.floor(np.log2(16384 // F)))
    pieces = -(-case["n"] // 1024)
    out = []
    for l, r in enumerate(case["res"]):
        dense = bool(ohash.level_is_dense(int(r), T, dim))
        rows = min(T, int(r) ** dim)
        buckets = -(-rows // centries)
        _, idx = ohash.corner_setup(case["coords"], int(r), T)
        out.append(dict(res=int(r), dense=dense, rows=rows, bucket_entries=centries, buckets=buckets,
                        owners=max(1, min(64 // buckets, pieces)), odd_start=bool(int(case["first_idx"][l]) & 1),
                        spill=bool((idx >= rows).any()), live=l * F < case["zero_from_col"]))
    return out


def reaches(case):
    """what a case reaches, decided on the host from level_is_dense, the row counts and the dispatch rules of launch_bwd:
    dense / hashed (a live level of that kind), multi_bucket (a dense level with at least two buckets: strips are dealt),
    sub_bucket (a level with fewer rows than one bucket), one_owner (a hashed level whose buckets have one reduce workgroup each),
    split (a level whose buckets are split over workgroups), odd_start, spill, dead_levels, and for the backward launch: merge,
    emit_lds_over (the emit kernel's LDS request is over 150 KiB), binned / direct, compact / generic (record form and emitter),
    collisions (a sample with two corners in one row of a hashed level), even_odd_x (hashed-level cells with even and odd x)"""
    F, dim, L = case["F"], case["dim"], case["L"]
    geo = [g for g in bin_geometry(case) if g["live"]]
    out = set()
    for g in geo:
        out.add("dense" if g["dense"] else "hashed")
        if g["dense"] and g["buckets"] >= 2:
            out.add("multi_bucket")
        if g["rows"] < g["bucket_entries"]:
            out.add("sub_bucket")
        if not g["dense"] and g["owners"] == 1:
            out.add("one_owner")
        if g["owners"] > 1:
            out.add("split")
        if g["odd_start"]:
            out.add("odd_start")
        if g["spill"]:
            out.add("spill")
    if len(geo) < L:
        out.add("dead_levels")
    W = F * (4 if case["dtype"] == "f32" else 2) // 4
    merge = F * (1 << dim) <= 32
    lds = (sum(g["buckets"] for g in geo) + 1 + 1024 * ((L * W) | 1)) * 4
    if merge:
        out.add("merge")
    if lds > 150 * 1024:
        out.add("emit_lds_over")
    out.add("binned" if merge and lds <= 150 * 1024 and case["n"] >= 4096 else "direct")
    out.add("compact" if case["dtype"] != "f32" and F == 2 else "generic")
    T = 2 ** case["bitwidth"]
    for l, r in enumerate(case["res"]):
        if not ohash.level_is_dense(r, T, dim):
            _, idx = ohash.corner_setup(case["coords"], r, T)
            if bool((idx.sort(1).values.diff(dim=1) == 0).any()):
                out.add("collisions")
            x0 = torch.floor((case["coords"][:, 0].double() * 0.5 + 0.5) * r).long()
            if bool((x0 % 2 == 0).any()) and bool((x0 % 2 == 1).any()):
                out.add("even_odd_x")
    return out


# ---------------------------------------------------------------------------------------------------- samples
def _lay_runs(n, runs):
    out, r = [], 0
    while len(out) < n:
        out += [r] * runs[r % len(runs)]
        r += 1
    return np.asarray(out[:n])


def max_numerator(res, b):
    """largest (p 2^b + k) a sample may have per axis: below res - 1 on every level under 258; everything up to c = +1 otherwise"""
    Rf = max(res)
    small = [r for r in res if r < 258]
    if not small:
        return Rf << b
    return ((Rf - Rf // min(small)) << b) - 1


def make_samples(dim, res, n, b=1, seed=0, runs=RUNS, plus_one=0):
    """numerators m [n, dim] (c = m / (Rf 2^b) * 2 - 1) and the run of every sample: runs of equal finest cells laid end to end
    without padding, so that runs start at arbitrary lanes (`reordered` gives the other orders).  plus_one: every plus_one-th run
    lies at c = +1 on all axes, the run after it on axis 0 only (needs every level at 258 or more)."""
    rng = np.random.default_rng(seed)
    Rf = max(res)
    run = _lay_runs(n, runs)
    nruns = int(run[-1]) + 1
    top = max_numerator(res, b)
    cells = rng.integers(0, (top >> b) + 1, size=(nruns, dim))
    k = rng.integers(0, 2 ** b, size=(n, dim))
    k[::5] = 0                                                    # offset 0: weights of exactly 1 and 0
    m = (cells[run] << b) + k
    m = np.minimum(m, top)
    if plus_one:
        assert top == Rf << b, "c = +1 needs every level at 258 or more"
        full = (run % plus_one) == 0
        m[full] = Rf << b
        m[((run % plus_one) == 1), 0] = Rf << b
    return m, run


def coords_of(m, res, b):
    c64 = m.astype(F64) / float(max(res) << b) * 2.0 - 1.0
    c32 = c64.astype(np.float32)
    assert np.array_equal(c32.astype(F64), c64), "inputs are not exact: a coordinate is not an fp32 value"
    return torch.from_numpy(c32)


def _ints(rng, shape, lo, hi):
    return rng.integers(lo, hi + 1, size=shape).astype(F64)


def make_grads(n, width, gmax, seed):
    """non-zero integers of magnitude 1 .. gmax, three in four positive (a row that cancels to exactly 0 cannot show a dropped
    record; a sum of one sign cannot show a wrong sign)"""
    rng = np.random.default_rng(seed + 5)
    mag = _ints(rng, (n, width), 1, gmax)
    sign = np.where(rng.integers(0, 4, size=(n, width)) == 0, -1.0, 1.0)
    return mag * sign


def make_case(name, dim, res, bitwidth, F, dtype="f32", n=1000, b=1, seed=0, gmax=2, tmax=3, scale_exp=0,
              pad=None, zero_from_col=None, plus_one=0, claims=(), samples=None, kind="bwd"):
    """One exact case on the CPU (not yet checked: reference_backward / reference_forward do that)."""
    res = [int(r) for r in res]
    L = len(res)
    sizes, first = layout(res, bitwidth, dim, pad)
    rows = int(first[L])
    m, run = samples if samples is not None else make_samples(dim, res, n, b, seed, plus_one=plus_one)
    n = m.shape[0]
    rng = np.random.default_rng(seed + 1)
    g = make_grads(n, L * F, gmax, seed) * 2.0 ** scale_exp
    td = DTYPES[dtype]
    g32 = torch.from_numpy(g).float()
    assert torch.equal(g32.to(td).double(), torch.from_numpy(g)), f"inputs are not exact: a gradient is not a {dtype} value"
    table = torch.from_numpy(_ints(rng, (rows, F), -tmax, tmax))
    ridx = np.arange(rows * F).reshape(rows, F)
    seeds = torch.from_numpy(((ridx * 7 + 3) % 11 - 5).astype(F64))
    return dict(name=name, kind=kind, dim=dim, res=res, bitwidth=bitwidth, F=F, dtype=dtype, n=n, b=b, L=L, rows=rows, sizes=sizes,
                first_idx=torch.from_numpy(np.asarray(first, dtype=np.int64)), m=m, run=run, coords=coords_of(m, res, b),
                grad_out=torch.from_numpy(g), table=table, seeds=seeds, scale_exp=scale_exp, gmax=gmax,
                zero_from_col=L * F if zero_from_col is None else int(zero_from_col), claims=tuple(claims), order="runs")


def reordered(case, order, seed=0):
    """the same multiset of samples (coordinates and gradient rows together) in another order: 'perm' (a random permutation) or
    'alt' (dealt round-robin over the runs: the k-th sample of every run in turn, so that neighbours lie in different cells and
    nothing merges on the finest level)"""
    n = case["n"]
    if order == "perm":
        p = np.random.default_rng(seed + 77).permutation(n)
    else:
        assert order == "alt"
        run = case["run"]
        start = np.concatenate([[0], np.flatnonzero(np.diff(run)) + 1])
        p = np.lexsort((run, np.arange(n) - start[run]))
    out = dict(case)
    out["m"], out["run"] = case["m"][p], case["run"][p]
    pt = torch.from_numpy(p)
    out["coords"], out["grad_out"] = case["coords"][pt].contiguous(), case["grad_out"][pt].contiguous()
    out["order"] = order
    out["name"] = f"{case['name']}/{order}"
    return out


def scaled(case, exp):
    """the same case with every gradient times 2^exp"""
    out = dict(case)
    out["grad_out"] = case["grad_out"] * 2.0 ** exp
    out["scale_exp"] = case["scale_exp"] + exp
    out["name"] = f"{case['name']}*2^{exp}"
    td = DTYPES[case["dtype"]]
    assert torch.equal(out["grad_out"].float().to(td).double(), out["grad_out"]), "inputs are not exact: a scaled gradient overflows"
    return out


# ---------------------------------------------------------------------------------------------------- weights
def level_weights(case, l):
    """-> (w float64 [n, 2^dim], idx int64 [n, 2^dim], cell id int64 [n], u): the oracle's fp32 weights and indices of level l,
    after asserting that they equal the float64 ones and lie on the level's grid of spacing u"""
    r, dim, b = case["res"][l], case["dim"], case["b"]
    Rf = max(case["res"])
    assert r & (r - 1) == 0, "resolutions are powers of two"
    d = int(np.log2(Rf // r))
    u = 2.0 ** (-dim * (b + d))
    c = case["coords"]
    assert np.array_equal(coords_of(case["m"], case["res"], b).numpy(), c.numpy()), "inputs are not exact: an offset has too many bits"
    coeffs, idx = ohash.corner_setup(c, r, 2 ** case["bitwidth"])
    x = (c.double() * 0.5 + 0.5) * float(r)
    assert torch.equal(x.float().double(), x), "inputs are not exact: a scaled position rounds in fp32"
    hi = float(np.float32(r - 1 - 1e-5))
    if r < 258:
        assert float(x.max()) < r - 1 and float(x.max()) <= hi, f"inputs are not exact: a coordinate is clamped at res {r} < 258"
    else:
        assert hi == float(r - 1)
        x = torch.clamp(x, max=float(r - 1))
    assert float(x.min()) >= 0.0
    pos = torch.floor(x)
    f = x - pos
    g = 1.0 - f
    w = torch.ones(c.shape[0], 1 << dim, dtype=torch.float64)
    for j in range(1 << dim):
        for a in range(dim):
            w[:, j] *= f[:, a] if (j >> (dim - 1 - a)) & 1 else g[:, a]
    assert torch.equal(coeffs.double(), w), f"inputs are not exact: a weight of res {r} rounds in fp32"
    assert torch.equal(torch.round(w / u) * u, w), f"a weight of res {r} is off the level's grid"
    cell = pos[:, 0].to(torch.int64)
    for a in range(1, dim):
        cell = cell * (r + 1) + pos[:, a].to(torch.int64)
    return w, idx, cell, u


def _tile_cell_max(w, gabs, cell):
    """max over (64-sample tile, cell, corner) of sum max_k |g_k| w: bounds every record the run merge can form (a run lies in ONE
    cell of one tile, so its corner sums are part of these)"""
    n = w.shape[0]
    key = (torch.arange(n) // TILE) * (int(cell.max()) + 1) + cell
    _, inv = torch.unique(key, return_inverse=True)
    s = torch.zeros(int(inv.max()) + 1, w.shape[1], dtype=torch.float64).index_add_(0, inv, w * gabs.max(1, keepdim=True).values)
    return float(s.max())


# ---------------------------------------------------------------------------------------------------- backward
def reference_backward(case, check=True):
    """float64 scatter-add of w_j g into row first_idx[l] + idx_j (dropped past the table), all levels below zero_from_col.
    -> dict(grad f64 [rows, F] (unseeded), zero_share [L] (None for dead levels), max_quanta, max_record_quanta)"""
    L, F, dim = case["L"], case["F"], case["dim"]
    rows = case["rows"]
    first = case["first_idx"]
    gunit = 2.0 ** case["scale_exp"]
    compact = case["dtype"] != "f32" and F == 2
    grad = torch.zeros(rows, F, dtype=torch.float64)
    zero_share, worst, worst_rec = [], 0.0, 0.0
    units, records = [], []
    for l in range(L):
        if l * F >= case["zero_from_col"]:
            zero_share.append(None)
            continue
        w, idx, cell, u = level_weights(case, l)
        g = case["grad_out"][:, l * F:(l + 1) * F].clone()
        for k in range(F):
            if l * F + k >= case["zero_from_col"]:
                g[:, k] = 0.0
        r = (int(first[l]) + idx).reshape(-1)
        keep = r < rows
        contrib = (w[:, :, None] * g[:, None, :]).reshape(-1, F)
        lvl = torch.zeros(rows, F, dtype=torch.float64).index_add_(0, r[keep], contrib[keep])
        grad += lvl
        if check:
            q = u * gunit
            asum = torch.zeros(rows, F, dtype=torch.float64).index_add_(0, r[keep], contrib[keep].abs())
            hits = torch.zeros(rows, dtype=torch.float64).index_add_(0, r[keep], (w.reshape(-1)[keep] != 0).double())
            assert torch.equal(torch.round(contrib / q) * q, contrib), f"level {l}: a product is off the grid of spacing {q}"
            quanta = (float(asum.max()) + (5.0 if case["scale_exp"] == 0 else 0.0)) / q
            assert quanta < 2.0 ** 24, f"inputs are not exact: sum |g| w = 2^{np.log2(quanta):.1f} quanta at level {l} (2^24 bound)"
            worst = max(worst, quanta)
            rec = _tile_cell_max(w, g.abs(), cell)
            if compact:
                assert rec / q < 2.0 ** 17, (f"inputs are not exact: a compact record of level {l} can reach 2^{np.log2(rec / q):.1f} "
                                             f"quanta (2^17 bound)")
            worst_rec = max(worst_rec, rec / q)
            units.append(q); records.append(rec)
            touched = hits > 0
            live = min(F, case["zero_from_col"] - l * F)                      # (columns cut by zero_from_col carry no gradient)
            zero_share.append(float(((lvl[:, :live] == 0) & touched[:, None]).sum()) / max(int(touched.sum()) * live, 1))
        else:
            zero_share.append(None)
    if check:
        # binary point of AccFix64: units of (largest record) * 2^-38, one bit coarser per doubling of the launch beyond 2^21
        extra = 0
        while (1 << (21 + extra)) < case["n"]:
            extra += 1
        assert min(units) >= max(records) * 2.0 ** (-38 + extra), "the smallest unit is below the fixed-point binary point"
        assert torch.equal(grad.float().double(), grad), "a gradient is not an fp32 value"
        if case["scale_exp"] == 0:
            assert torch.equal((grad + case["seeds"]).float().double(), grad + case["seeds"])
    return dict(grad=grad, zero_share=zero_share, max_quanta=worst, max_record_quanta=worst_rec)


# ---------------------------------------------------------------------------------------------------- forward
def reference_forward(case, check=True):
    """float64 lookup, rounded once to the table's type; -> tensor [n, L F] of that type"""
    L, F = case["L"], case["F"]
    first, rows = case["first_idx"], case["rows"]
    td = DTYPES[case["dtype"]]
    table = case["table"]
    assert torch.equal(table.float().to(td).double(), table), "inputs are not exact: a table value is not of the table's type"
    out = torch.zeros(case["n"], L * F, dtype=torch.float64)
    for l in range(L):
        if l * F >= case["zero_from_col"]:
            continue
        w, idx, _, u = level_weights(case, l)
        r = torch.clamp(int(first[l]) + idx, max=rows - 1)
        v = table[r]                                                 # [n, 2^dim, F]
        s = (w[:, :, None] * v).sum(1)
        if check:
            mag = (w[:, :, None] * v.abs()).sum(1)
            assert float(mag.max()) / u < 2.0 ** 24, f"level {l}: a per-level sum has more than 24 significant bits"
            assert torch.equal(s.float().double(), s)
        out[:, l * F:(l + 1) * F] = s
    out[:, case["zero_from_col"]:] = 0.0
    # (at most 24 significant bits: double -> float is exact, float -> half / bfloat16 rounds once)
    return out.float().to(td)


# ---------------------------------------------------------------------------------------------------- grad_coords
def reference_grad_coords(case, check=True):
    """oracle.hashgrid.hashgrid_grad_coords restated in float64, quirks kept: every level reads the upstream gradient of the FIRST
    level's columns, d/dy ends with (corner 7 - corner 6), no factor res / 2; 2-D: zeros [n, 3]."""
    n, L, F, dim = case["n"], case["L"], case["F"], case["dim"]
    out = torch.zeros(n, 3, dtype=torch.float64)
    if dim != 3:
        return out.float()
    mag = torch.zeros(n, 3, dtype=torch.float64)
    go, table, first = case["grad_out"], case["table"], case["first_idx"]
    umin = 1.0
    for l in range(L):
        r = case["res"][l]
        _, idx, _, u = level_weights(case, l)
        umin = min(umin, u)
        x = (case["coords"].double() * 0.5 + 0.5) * float(r)
        if r >= 258:
            x = torch.clamp(x, max=float(r - 1))
        f = x - torch.floor(x)
        g = 1.0 - f
        base = int(first[l])
        for j in range(F):
            v = [table[base + idx[:, k], j] for k in range(8)]
            wj = go[:, j]
            tx = ((g[:, 1] * g[:, 2]) * (v[4] - v[0]), (g[:, 1] * f[:, 2]) * (v[5] - v[1]),
                  (f[:, 1] * g[:, 2]) * (v[6] - v[2]), (f[:, 1] * f[:, 2]) * (v[7] - v[3]))
            ty = ((g[:, 0] * g[:, 2]) * (v[2] - v[0]), (g[:, 0] * f[:, 2]) * (v[3] - v[1]),
                  (f[:, 0] * g[:, 2]) * (v[6] - v[4]), (f[:, 0] * f[:, 2]) * (v[7] - v[6]))
            tz = ((g[:, 0] * g[:, 1]) * (v[1] - v[0]), (g[:, 0] * f[:, 1]) * (v[3] - v[2]),
                  (f[:, 0] * g[:, 1]) * (v[5] - v[4]), (f[:, 0] * f[:, 1]) * (v[7] - v[6]))
            for a, t in enumerate((tx, ty, tz)):
                out[:, a] += wj * (t[0] + t[1] + t[2] + t[3])
                mag[:, a] += wj.abs() * (t[0].abs() + t[1].abs() + t[2].abs() + t[3].abs())
    if check:
        q = umin * 2.0 ** case["scale_exp"]
        assert float(mag.max()) / q < 2.0 ** 24, "inputs are not exact: a grad_coords sum leaves 24 bits"
        assert torch.equal(out.float().double(), out)
    return out.float()


# ---------------------------------------------------------------------------------------------------- corner query
def make_query_case(dtype, probe_bitwidth, n=300, res=(16, 64, 512), bitwidth=12, F=2, seed=0, gmax=2):
    """coordinates as above (3-D), one gradient table [2^bitwidth, F] per level, grad_out [n, 8, L, P, F] of non-zero integers"""
    res = [int(r) for r in res]
    m, run = make_samples(3, res, n, 1, seed + 31, runs=(1, 2, 3, 5))
    L, P = len(res), 2 ** probe_bitwidth
    g = make_grads(n, 8 * L * P * F, gmax, seed + 9).reshape(n, 8, L, P, F)
    return dict(name=f"query {dtype} probe {probe_bitwidth}", dtype=dtype, res=res, bitwidth=bitwidth, F=F, n=n, L=L, P=P, b=1, m=m,
                probe_bitwidth=probe_bitwidth, coords=coords_of(m, res, 1), grad_out=torch.from_numpy(g))


def reference_query_backward(case, check=True):
    """oracle.hashgrid.hashgrid_query_backward in float64 -> list of tables of the gradient's type.  fp32: probe p into row
    idx + p; 16 bit: every probe into row idx, and the packed atomics round every partial sum - so sum |g| per entry stays within
    the integers the type holds exactly (2048 for fp16, 256 for bf16)."""
    half = case["dtype"] != "f32"
    td = DTYPES[case["dtype"]]
    args = (case["coords"], case["grad_out"], case["res"], case["bitwidth"], case["F"], case["probe_bitwidth"], half)
    want = ohash.hashgrid_query_backward(*args, acc_dtype=torch.float64)
    if check:
        mags = ohash.hashgrid_query_backward(case["coords"], case["grad_out"].abs(), *args[2:], acc_dtype=torch.float64)
        limit = {"f32": 2.0 ** 24, "f16": 2048.0, "bf16": 256.0}[case["dtype"]]
        worst = max(float(t.max()) for t in mags)
        assert worst <= limit, f"inputs are not exact: sum |g| = {worst} on one entry ({case['dtype']} holds integers to {limit})"
        assert any(int((t != 0).sum()) > 0 for t in want)
    return [t.float().to(td) for t in want]


# ---------------------------------------------------------------------------------------------------- the case lists
R3 = (16, 32, 64)                    # 3-D at bitwidth 16: res 16 below one bucket, res 32 dense with 4 buckets (F = 2), res 64 hashed
R3W = (8, 16, 32, 64)
R2 = (64, 128, 256, 512)             # 2-D at bitwidth 14: 64 dense, 128 .. 512 hashed
N_DIRECT, N_BINNED = 4095, 4096


def _bwd(name, dim, res, bw, F, dtype, n, claims=(), **kw):
    gmax = kw.pop("gmax", 2 if (dtype != "f32" and F == 2) else 4)
    return make_case(name, dim, res, bw, F, dtype, n=n, gmax=gmax, claims=claims, kind="bwd", seed=kw.pop("seed", len(name) + n), **kw)


_BWD_SPECS = [
    # name, builder arguments; claims are verified by tests/test_hashgrid_exact_host.py
    ("direct f32 F2 n4095", dict(dim=3, res=R3W, bw=16, F=2, dtype="f32", n=N_DIRECT, claims=("dense", "hashed"))),
    ("generic f32 F2 n4096", dict(dim=3, res=R3W, bw=16, F=2, dtype="f32", n=N_BINNED, claims=("dense", "hashed", "multi_bucket", "sub_bucket", "split"))),
    ("generic f32 F4 n4097", dict(dim=3, res=R3W, bw=16, F=4, dtype="f32", n=4097, claims=("multi_bucket",))),
    ("generic f16 F4 n5000", dict(dim=3, res=R3W, bw=16, F=4, dtype="f16", n=5000, claims=("hashed",))),
    ("generic bf16 F4 n8193", dict(dim=3, res=R3W, bw=16, F=4, dtype="bf16", n=8193, claims=("hashed",))),
    ("generic f32 F2 n8193", dict(dim=3, res=R3W, bw=16, F=2, dtype="f32", n=8193, claims=("multi_bucket",))),
    ("generic f32 F2 n5000", dict(dim=3, res=R3W, bw=16, F=2, dtype="f32", n=5000, claims=("multi_bucket",))),
    ("compact f16 F2 3d n4096", dict(dim=3, res=R3, bw=16, F=2, dtype="f16", n=4096, claims=("dense", "hashed", "multi_bucket", "sub_bucket"))),
    ("compact bf16 F2 3d n4097", dict(dim=3, res=R3, bw=16, F=2, dtype="bf16", n=4097, claims=("multi_bucket", "sub_bucket"))),
    ("compact bf16 F2 3d n5000", dict(dim=3, res=R3, bw=16, F=2, dtype="bf16", n=5000, claims=("multi_bucket",))),
    ("compact f16 F2 3d n8193", dict(dim=3, res=R3, bw=16, F=2, dtype="f16", n=8193, claims=("multi_bucket",))),
    ("compact direct bf16 F2 3d n4095", dict(dim=3, res=R3, bw=16, F=2, dtype="bf16", n=N_DIRECT, claims=("dense", "hashed"))),
    ("compact f16 F2 2d n5000", dict(dim=2, res=R2, bw=14, F=2, dtype="f16", n=5000, claims=("dense", "hashed", "sub_bucket"))),
    ("compact bf16 F2 2d n5000", dict(dim=2, res=R2, bw=14, F=2, dtype="bf16", n=5000, claims=("dense", "hashed"))),
    ("no merge f32 F8 3d n5000", dict(dim=3, res=R3, bw=16, F=8, dtype="f32", n=5000, claims=("dense", "hashed"))),
    ("no merge bf16 F16 3d n5000", dict(dim=3, res=R3, bw=16, F=16, dtype="bf16", n=5000, claims=("dense", "hashed"))),
    ("merge f32 F8 2d one owner n6000", dict(dim=2, res=(128, 256, 512), bw=17, F=8, dtype="f32", n=6000, claims=("dense", "hashed", "one_owner", "multi_bucket"))),
    ("no bins f32 F4 12 levels n5000", dict(dim=3, res=(8, 8, 16, 16, 16, 32, 32, 32, 64, 64, 64, 64), bw=14, F=4, dtype="f32", n=5000,
                                           claims=("dense", "hashed", "emit_lds_over"))),
    ("odd start f32 F2 n5000", dict(dim=3, res=R3, bw=16, F=2, dtype="f32", n=5000, pad=(0, 1, 2), claims=("odd_start", "multi_bucket"))),
    ("odd start bf16 F2 n5000", dict(dim=3, res=R3, bw=16, F=2, dtype="bf16", n=5000, pad=(3, 2, 1), claims=("odd_start",))),
    ("dead suffix bf16 F2 n5000", dict(dim=3, res=R3, bw=16, F=2, dtype="bf16", n=5000, zero_from_col=4, claims=("dead_levels",))),
    ("dead suffix f32 F4 n5000", dict(dim=3, res=R3W, bw=16, F=4, dtype="f32", n=5000, zero_from_col=10, claims=("dead_levels",))),
    ("spill f32 F2 2d n5000", dict(dim=2, res=(512, 1024, 512), bw=21, F=2, dtype="f32", n=5000, plus_one=7, claims=("dense", "spill", "multi_bucket"))),
    ("spill bf16 F2 2d n5000", dict(dim=2, res=(512, 1024, 512), bw=21, F=2, dtype="bf16", n=5000, plus_one=7, claims=("dense", "spill"))),
]
BWD_NAMES = [s[0] for s in _BWD_SPECS]
BIG_SPECS = [
    ("big bf16 F2 wide emitter", dict(dim=3, res=(32, 128), bw=16, F=2, dtype="bf16", n=(1 << 20) + 2048 + 17, gmax=1, claims=("multi_bucket", "hashed"))),
    ("big f32 F2 extra bit", dict(dim=3, res=(32, 128), bw=16, F=2, dtype="f32", n=(1 << 21) + 65, gmax=1, claims=("multi_bucket", "hashed"))),
]
BIG_NAMES = [s[0] for s in BIG_SPECS]
# For the AdamW step folded into the reduce kernel's flush (tests/test_gpu_optim_exact.py; claims verified by
# tests/test_optim_exact_host.py).  The fold exists for F = 2 and covers a level whose buckets have ONE reduce workgroup each: with
# 5 emitting pieces that takes more than 32 buckets of 8192 rows, i.e. 2^19 rows or more.  2-D: res 512 is dense with 32 buckets
# (split: not covered); res 1024 is dense at bitwidth 21 (128 buckets of strips, one owner) and hashed at bitwidth 19 (64 buckets,
# one owner).
ADAM_SPECS = [
    ("adam dense one owner f32 F2 2d n5000", dict(dim=2, res=(512, 1024), bw=21, F=2, dtype="f32", n=5000, pad=(3, 2), claims=("dense", "multi_bucket", "split", "odd_start"))),
    ("adam hashed one owner f32 F2 2d n5000", dict(dim=2, res=(512, 1024), bw=19, F=2, dtype="f32", n=5000, claims=("dense", "hashed", "one_owner", "split"))),
    ("adam dead suffix bf16 F2 2d n5000", dict(dim=2, res=(512, 1024, 512), bw=19, F=2, dtype="bf16", n=5000, pad=(1, 2, 0), zero_from_col=4,
                                               claims=("dead_levels", "hashed", "one_owner", "compact", "odd_start"))),
]
ADAM_NAMES = [s[0] for s in ADAM_SPECS]
LOSS_SCALES = (16, 24, -30)
LOSS_NAMES = ("generic f32 F2 n5000", "compact bf16 F2 3d n5000", "compact f16 F2 3d n8193", "generic f16 F4 n5000")
F16_UNIT_EXP = -10                  # fp16 cannot hold 2^16: its loss-scale cases start from integers times 2^-10
ORDER_NAMES = ("generic f32 F2 n5000", "compact bf16 F2 3d n5000")

_cases = {}


def bwd_case(name):
    if name not in _cases:
        spec = dict(dict(_BWD_SPECS + BIG_SPECS + ADAM_SPECS)[name])
        _cases[name] = _bwd(name, spec.pop("dim"), spec.pop("res"), spec.pop("bw"), spec.pop("F"), spec.pop("dtype"), spec.pop("n"),
                            spec.pop("claims"), **spec)
    return _cases[name]


def loss_scale_cases(name):
    """[(case, exponent)]: the same integer gradients times 2^16, 2^24 and 2^-30 (fp16: from a unit of 2^-10, and no 2^-30)"""
    base = bwd_case(name)
    out = []
    for e in LOSS_SCALES:
        if base["dtype"] == "f16":
            if e < 0:
                continue
            limited = dict(base)
            limited["grad_out"] = base["grad_out"].clamp(-2, 2)
            out.append((scaled(limited, e + F16_UNIT_EXP), e))
        else:
            out.append((scaled(base, e), e))
    return out


FWD_DTYPES = ("f32", "f16", "bf16")
FWD_F = (2, 4, 8, 16)
FWD_LAYOUTS = {2: dict(res4=(64, 128, 256, 512), res5=(32, 64, 128, 256, 512), bw=14), 3: dict(res4=(8, 16, 32, 64), res5=(8, 16, 32, 32, 64), bw=14)}
FWD_SMALL_N = (1, 63, 64, 65, 257)
FWD_WIDTHS = {1: ("bf16", 2), 2: ("f32", 2), 4: ("f32", 4), 8: ("f32", 8), 16: ("f32", 16)}       # row width W in dwords -> (dtype, F)


def fwd_case(dtype, F, dim, lods, n=1000, **kw):
    lay = FWD_LAYOUTS[dim]
    key = ("fwd", dtype, F, dim, lods, n, tuple(sorted((k, str(v)) for k, v in kw.items())))
    if key not in _cases:
        res = kw.pop("res", lay["res4"] if lods == 4 else lay["res5"])
        _cases[key] = make_case(f"fwd {dtype} F{F} {dim}d L{len(res)} n{n}", dim, res, kw.pop("bw", lay["bw"]), F, dtype, n=n, kind="fwd",
                                seed=kw.pop("seed", 3 * F + dim + n), claims=kw.pop("claims", ("dense", "hashed")), **kw)
    return _cases[key]


def fwd_tiny_case(dtype, bw, dim):
    """tiny tables for the 16-bit F = 2 pair loads: heavy collisions (several corners of a sample in one row), even and odd cell x"""
    res = (8, 16, 32) if dim == 3 else (8, 16, 32, 64)
    claims = ("hashed", "even_odd_x") + (("collisions",) if bw == 1 or dim == 3 else ())   # (four corners in 64 rows rarely meet)
    return fwd_case(dtype, 2, dim, len(res), n=777, res=res, bw=bw, claims=claims)


def fwd_spill_cases():
    """2-D dense levels at bitwidth 21.  res 256 is below 258 (its clamp bound is not dyadic), so c = +1 cannot be exact with it:
    256 / 512 / 1024 run without c = +1, and 512 / 1024 / 512 with c = +1 on every axis (level 0 spills into level 1, level 1 into
    level 2, level 2 - the last - onto the table's last row)."""
    a = [fwd_case(dt, 2, 2, 3, n=1000, res=(256, 512, 1024), bw=21, claims=("dense",)) for dt in ("f32", "bf16")]
    b = [fwd_case(dt, 2, 2, 3, n=1000, res=(512, 1024, 512), bw=21, plus_one=5, claims=("dense", "spill")) for dt in ("f32", "f16", "bf16")]
    return a + b


FWD_CUT = (("bf16", 2), ("f32", 4), ("f16", 8))


def fwd_cut_cases(dtype, F):
    """zero_from_col after level 0, inside level 2 and at L F"""
    base = fwd_case(dtype, F, 3, 4)
    out = []
    for cut in (F, 2 * F + 1, 4 * F):
        case = dict(base)
        case["zero_from_col"] = cut
        case["name"] = f"{base['name']} cut {cut}"
        case["claims"] = base["claims"] if cut == 4 * F else ("dense", "dead_levels")
        out.append(case)
    return out


def fwd_cases_all():
    """every forward case of the GPU file (for the host test)"""
    out = []
    for dim in (2, 3):
        for dt in FWD_DTYPES:
            for F in FWD_F:
                for lods in (4, 5):
                    out.append(fwd_case(dt, F, dim, lods))
    for W, (dt, F) in FWD_WIDTHS.items():
        for n in FWD_SMALL_N:
            out.append(fwd_case(dt, F, 3, 5, n=n, claims=()))
    for dt in ("f16", "bf16"):
        for bw in (1, 6):
            for dim in (2, 3):
                out.append(fwd_tiny_case(dt, bw, dim))
    for dt, F in (("bf16", 2), ("f32", 2)):
        out.append(fwd_case(dt, F, 3, 4, n=1000, pad=(0, 1, 2, 0), claims=("odd_start",)))
    for dt, F in FWD_CUT:
        out += fwd_cut_cases(dt, F)
    out += fwd_spill_cases()
    return out


GC_N = (1, 255, 256, 257)


def grad_coords_case(dtype, F, n, dim=3):
    key = ("gc", dtype, F, n, dim)
    if key not in _cases:
        res = (8, 16, 32, 64) if dim == 3 else (64, 128, 256)
        _cases[key] = make_case(f"grad_coords {dtype} F{F} n{n}", dim, res, 14, F, dtype, n=n, gmax=2, tmax=3, seed=n + F, kind="gc")
    return _cases[key]
