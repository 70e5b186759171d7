"""float64 restatement of the fused image training step (csrc/image_field_train.hip: forward, loss = F.mse_loss(pred, rgb) and all
five gradients), and a generator of exactly representable training cases.  Test infrastructure only; host only (numpy + torch CPU),
over oracle/hashgrid.py with 2-D coordinates.

A field is a dict: table f32 [rows, 2], begin int64 [L + 1], resolutions, bitwidth, active (the number of levels rgb() blends: 'cat'
leaves the columns of the levels from `active` on zero), w1 [H, 2 L + 14], b1 [H], w2 [3, H], b2 [3].

The gradients are written out, not taken from autograd: with x = [features, embedding], a = W1 x + b1, h = relu(a), o = W2 h + b2,
s = sigmoid(o), d = s - t, g = 2 d / (3 n), dO = g s (1 - s):  d b2 = sum dO,  d W2 = dO^T h,  dh = dO W2 [a > 0],  d b1 = sum dh,
d W1 = dh^T x,  d features = dh W1[:, :2 L], and the table gradient is a float64 index_add_ of blend factor * d features over the four
corner rows of every active level.

Exact cases: "twin levels".  A sigmoid ruins exactness unless every output is exactly 0 (s = 1/2, s (1 - s) = 1/4), so the outputs
are made to cancel: active levels come in pairs of equal resolution with identical table contents (same resolution, same hash ->
bitwise equal feature columns), hidden units in pairs (2 i, 2 i + 1) that read one feature column of a level / the same column of
its twin with the same weight +-1 and the same small-integer bias, the embedding columns of W1 are zero, W2[:, 2 i + 1] =
-W2[:, 2 i] with entries in {-1, 0, 1} and b2 = 0.  Coordinates are -1 + 2 m / D (D = 64, or 8 x the coarsest resolution when that
is smaller) below every level's clamp, so blend factors are dyadic with at most 6 bits; targets are 1/2 - 3 m_k / 16 with m_k in
-2 .. 2, so for n a power of two g = m_k / (8 n) exactly.  Tables hold integers in [-1, 1].  check_exact proves per case that every term of every sum is a
multiple of one quantum and that the sum of absolute values, pre-fill included, stays below 2^24 quanta IN ANY ORDER OF ADDITION: a
kernel must equal the float64 result BIT FOR BIT, float atomics or not.  A failure there blames the inputs, not the kernel.
The embedding columns of d W1 are not exact (dh * sin is not) and are left to the generic comparison.
"""
import numpy as np
import torch

from oracle import hashgrid as ohg

F64 = torch.float64
EMBED = 14
PREFILL_MAX = 2.0                      # |value| a gradient buffer may be pre-filled with (multiples of 1/2)
GRADS = ("table", "w1", "b1", "w2", "b2")


def layout(resolutions, bitwidth, coord_dim=2):
    """begin_idxes of the table: min(2^bitwidth, res^coord_dim) rows a level (coord_dim = 3 is what a HashGrid built with its
    default coord_dim declares, as the image application's is)"""
    return torch.from_numpy(ohg.table_layout(resolutions, 2 ** bitwidth, coord_dim)[1])


def level_corners(fld, coords):
    """per level (blend factors float64 [n, 4], table rows int64 [n, 4]) - the factors from the fp32 position the kernel forms"""
    T = 2 ** fld["bitwidth"]
    c32 = coords.float()
    out = []
    for l, res in enumerate(fld["resolutions"]):
        _, idx = ohg.corner_setup(c32, int(res), T)
        x = ((c32.double() * 0.5 + 0.5) * float(res)).float()
        x = torch.clamp(x, min=0.0, max=float(np.float32(res - 1 - 1e-5)))
        f = (x - torch.floor(x)).double()
        g = 1.0 - f
        w = torch.stack([(f if j & 2 else g)[:, 0] * (f if j & 1 else g)[:, 1] for j in range(4)], 1)
        out.append((w, int(fld["begin"][l]) + idx))
    return out


def embed(coords):
    """PositionalEmbedder's 14 columns from the fp32 coordinates, in float64: [x, y | sin(1x) sin(1y) sin(2x) .. | cos(same)]"""
    c = coords.float().double()
    args = torch.cat([c * float(2 ** f) for f in range(3)], dim=1)
    return torch.cat([c, torch.sin(args), torch.cos(args)], dim=1)


def features(fld, coords, table=None):
    """float64 [n, 2 L]: the 'cat' lookup, columns of the levels from `active` on zero (differentiable in `table`)"""
    table = fld["table"].double() if table is None else table
    cols = []
    for l, (w, rows) in enumerate(level_corners(fld, coords)):
        if l < fld["active"]:
            cols.append((table[rows.reshape(-1)].reshape(rows.shape[0], 4, 2) * w[:, :, None]).sum(1))
        else:
            cols.append(torch.zeros(coords.shape[0], 2, dtype=F64))
    return torch.cat(cols, dim=1)


def decoder_parts(fld, coords, rgb):
    """the float64 forward and decoder backward: dict of x, a, h, o, pred, d, g, do, dh, dfeat"""
    n, L2 = coords.shape[0], 2 * len(fld["resolutions"])
    x = torch.cat([features(fld, coords), embed(coords)], dim=1)
    w1, b1, w2, b2 = (fld[k].double() for k in ("w1", "b1", "w2", "b2"))
    a = x @ w1.T + b1
    h = torch.relu(a)
    o = h @ w2.T + b2
    s = 1.0 / (1.0 + torch.exp(-o))
    d = s - rgb.double()
    g = 2.0 * d / (3 * n)
    do = g * (s * (1.0 - s))
    dh = (do @ w2) * (a > 0)
    return dict(x=x, a=a, h=h, o=o, pred=s, d=d, g=g, do=do, dh=dh, dfeat=dh @ w1[:, :L2])


def step_reference(fld, coords, rgb):
    """float64: dict(loss [1], pred [n, 3], table, w1, b1, w2, b2) - the five gradients under their parameter's name"""
    assert fld["table"].dtype == torch.float32, "the table is f32 under training"
    p = decoder_parts(fld, coords, rgb)
    n = coords.shape[0]
    table = torch.zeros(fld["table"].shape, dtype=F64)
    corners = level_corners(fld, coords)
    for l in range(fld["active"]):
        w, rows = corners[l]
        dl = p["dfeat"][:, 2 * l:2 * l + 2]
        table.index_add_(0, rows.reshape(-1), (w[:, :, None] * dl[:, None, :]).reshape(-1, 2))
    return dict(loss=(p["d"] ** 2).sum().reshape(1) / (3 * n), pred=p["pred"], table=table, w1=p["dh"].T @ p["x"], b1=p["dh"].sum(0),
                w2=p["do"].T @ p["h"], b2=p["do"].sum(0))


def autograd_reference(fld, coords, rgb):
    """the same numbers from torch autograd in float64: F.mse_loss(sigmoid(decoder([features, embed])), rgb) through the 2-D oracle's
    corner indices"""
    leaves = {k: fld[k].double().clone().requires_grad_(True) for k in GRADS}
    x = torch.cat([features(fld, coords, leaves["table"]), embed(coords)], dim=1)
    o = torch.relu(x @ leaves["w1"].T + leaves["b1"]) @ leaves["w2"].T + leaves["b2"]
    pred = torch.sigmoid(o)
    loss = torch.nn.functional.mse_loss(pred, rgb.double())
    loss.backward()
    return dict(loss=loss.detach().reshape(1), pred=pred.detach(),
                **{k: (torch.zeros_like(v) if v.grad is None else v.grad) for k, v in leaves.items()})


# ---------------------------------------------------------------------------------------------------- generic fields
def geometric_resolutions(L, lo=16, hi=512):
    if L == 1:
        return [lo]
    b = np.exp((np.log(hi) - np.log(lo)) / (L - 1))
    return [int(np.floor(lo * b ** l)) for l in range(L)]


def generic_field(L, hidden, active, bitwidth, seed=0, coord_dim=2):
    """an image field with random parameters: resolutions 16 .. 512 in geometric steps, table entries N(0, 0.3), decoder weights of
    torch.nn.Linear's scale"""
    g = torch.Generator().manual_seed(1000 * seed + 37 * L + hidden)
    res = geometric_resolutions(L)
    begin = layout(res, bitwidth, coord_dim)
    in_dim = 2 * L + EMBED
    u = lambda *shape, k: (torch.rand(*shape, generator=g) * 2 - 1) * k
    return dict(table=torch.randn(int(begin[-1]), 2, generator=g) * 0.3, begin=begin, resolutions=res, bitwidth=int(bitwidth),
                active=int(active), w1=u(hidden, in_dim, k=in_dim ** -0.5), b1=u(hidden, k=in_dim ** -0.5),
                w2=u(3, hidden, k=max(hidden, 4) ** -0.5 * 2), b2=u(3, k=0.5))


def generic_points(n, seed=0):
    """coordinates in [-1, 1]^2; every 7th point has a coordinate outside (clamped to the border cell), every 5th lies on a cell
    face of resolution 16 (and 1 itself occurs)"""
    g = torch.Generator().manual_seed(77 + seed)
    c = torch.rand(n, 2, generator=g) * 2 - 1
    idx = torch.arange(n)
    face = idx % 5 == 4
    c[face, 0] = (torch.randint(0, 17, (int(face.sum()),), generator=g).float() / 8.0 - 1.0)
    out = idx % 7 == 6
    c[out, 1] = torch.where(torch.rand(int(out.sum()), generator=g) < 0.5, torch.tensor(-1.25), torch.tensor(1.5))
    return c


def generic_targets(n, seed=0):
    return torch.rand(n, 3, generator=torch.Generator().manual_seed(991 + seed))


# ---------------------------------------------------------------------------------------------------- exact cases
def twin_pairs(fld):
    """[(l, l + 1)] consecutive ACTIVE levels of equal resolution, each level in at most one pair"""
    res, pairs, l = fld["resolutions"], [], 0
    while l + 1 < fld["active"]:
        if res[l] == res[l + 1]:
            pairs.append((l, l + 1))
            l += 2
        else:
            l += 1
    return pairs


def exact_field(resolutions, active, bitwidth, hidden, seed=0, coord_dim=2):
    rng = np.random.default_rng(seed)
    L = len(resolutions)
    begin = layout(resolutions, bitwidth, coord_dim)
    table = torch.zeros(int(begin[-1]), 2)
    for l in range(L):
        rows = int(begin[l + 1] - begin[l])
        if l > 0 and resolutions[l] == resolutions[l - 1] and rows == int(begin[l] - begin[l - 1]):
            table[int(begin[l]):int(begin[l + 1])] = table[int(begin[l - 1]):int(begin[l])]              # the twin's contents
        else:
            table[int(begin[l]):int(begin[l + 1])] = torch.from_numpy(rng.integers(-1, 2, size=(rows, 2)).astype(np.float32))
    fld = dict(table=table, begin=begin, resolutions=[int(r) for r in resolutions], bitwidth=int(bitwidth), active=int(active))
    pairs = twin_pairs(fld)
    w1 = np.zeros((hidden, 2 * L + EMBED), dtype=np.float32)
    b1 = np.zeros(hidden, dtype=np.float32)
    w2 = np.zeros((3, hidden), dtype=np.float32)
    for i in range(hidden // 2):
        sign, bias = rng.choice([-1.0, 1.0]), float(rng.integers(-1, 2))
        if pairs:
            a, b = pairs[i % len(pairs)]
            k = int(rng.integers(0, 2))
            w1[2 * i, 2 * a + k] = sign
            w1[2 * i + 1, 2 * b + k] = sign
        b1[2 * i] = b1[2 * i + 1] = bias
        col = rng.integers(-1, 2, size=3).astype(np.float32)
        if not col.any():
            col[int(rng.integers(0, 3))] = 1.0
        w2[:, 2 * i], w2[:, 2 * i + 1] = col, -col
    if hidden % 2:                                           # an odd unit has no twin: it feeds no output
        b1[hidden - 1] = 1.0
    fld.update(w1=torch.from_numpy(w1), b1=torch.from_numpy(b1), w2=torch.from_numpy(w2), b2=torch.zeros(3))
    return fld


def exact_denominator(resolutions):
    """coordinates are -1 + 2 m / D: D = 64 (-1 + m / 32), or 8 x the coarsest resolution where that is smaller - a cell
    position then has at most 3 fractional bits on every level, a blend factor 6; on levels of resolution D and above every
    coordinate is a grid point (blend factors 1 and 0)"""
    return min(64, 8 * min(int(r) for r in resolutions))


def exact_points(n, resolutions, seed=0):
    """-1 + 2 m / D with m below every level's clamp and below 55 D / 64; the first points are fixed: a corner of the finest
    level's cell grid, a face of every level"""
    D = exact_denominator(resolutions)
    top = min(55 * D // 64, int(D * (1.0 - 1.0 / min(resolutions))) - 1)
    rng = np.random.default_rng(seed)
    m = rng.integers(0, top + 1, size=(n, 2))
    m[0] = (0, 0)
    if n > 1:
        m[1] = (D // 2, top)
    return torch.from_numpy((-1.0 + 2.0 * m / D).astype(np.float32))


def exact_targets(n, seed=0):
    rng = np.random.default_rng(seed + 5)
    mk = rng.integers(-2, 3, size=(n, 3))
    mk[0] = (2, -1, 1)                                        # (a single sample still has a gradient)
    return torch.from_numpy((0.5 - 3.0 * mk / 16.0).astype(np.float32))


def _budget(name, abs_sum, values, quantum, spans, extra=0.0):
    """every value is a multiple of `quantum`; the sum of absolute values (plus `extra`) stays below 2^24 quanta"""
    v = values.double()
    assert bool(torch.equal(torch.round(v / quantum) * quantum, v)), f"{name}: a term is off the quantum grid"
    top = (float(abs_sum.max()) if abs_sum.numel() else 0.0) + extra
    quanta = max(top / quantum, 1.0)
    assert quanta < 2.0 ** 24, f"{name}: the partial sums leave fp32 ({np.log2(quanta):.1f} bits)"
    spans[name] = quanta
    return quanta


def check_exact(fld, coords, rgb, prefill=PREFILL_MAX):
    """assert the exactness conditions of the whole step; returns {stage: largest abs-sum in quanta}"""
    n, L2 = coords.shape[0], 2 * len(fld["resolutions"])
    assert n >= 1 and n & (n - 1) == 0, "n must be a power of two: 2 d / (3 n) is exact"
    res = [fld["resolutions"][l] for l in range(fld["active"])] or [1]
    D = exact_denominator(fld["resolutions"])
    m = (coords.double() + 1.0) * D / 2.0
    assert bool(torch.equal(torch.round(m), m)), "coords: a coordinate is off the quantum grid"
    assert all(r & (r - 1) == 0 for r in res), "an active resolution is no power of two"
    fbits = max(int(np.log2(D // min(D, r))) for r in res)          # fractional bits of a cell position
    assert fbits <= 3
    q = 2.0 ** (-2 * fbits)                                          # quantum of a blend factor, a feature and a hidden unit
    for l in range(fld["active"]):
        x = (coords.double() * 0.5 + 0.5) * res[l]
        assert float(x.max()) < res[l] - 1 - 1e-5 and float(x.min()) >= 0, "a coordinate meets the clamp"
    assert bool(torch.equal(fld["table"], torch.round(fld["table"]))) and float(fld["table"].abs().max()) <= 1
    assert bool((fld["w1"][:, L2:] == 0).all()) and bool((fld["b2"] == 0).all())
    assert bool(torch.equal(fld["w1"].abs(), fld["w1"].abs() ** 2)) and bool(torch.equal(fld["w2"].abs(), fld["w2"].abs() ** 2))
    spans = {}
    p = decoder_parts(fld, coords, rgb)
    corners = level_corners(fld, coords)
    _budget("blend", torch.ones(1), torch.cat([w.reshape(-1) for w, _ in corners[:fld["active"]]] or [torch.zeros(1, dtype=F64)]), q, spans)
    _budget("hidden", p["x"][:, :L2].abs() @ fld["w1"].double().abs()[:, :L2].T + fld["b1"].double().abs(), p["a"], q, spans)
    # the outputs cancel unit pair by unit pair in the fp32 fma chain: equal pre-activations, opposite W2 columns
    H = fld["w1"].shape[0]
    even = slice(0, H - H % 2, 2)
    odd = slice(1, H, 2)
    assert bool(torch.equal(p["a"][:, even], p["a"][:, odd])) and bool(torch.equal(fld["w2"][:, even], -fld["w2"][:, odd]))
    assert H % 2 == 0 or bool((fld["w2"][:, H - 1] == 0).all())
    assert bool((p["o"] == 0).all()) and bool((p["pred"] == 0.5).all()), "an output is not exactly zero"
    mk = (0.5 - rgb.double()) * 16.0 / 3.0
    assert bool(torch.equal(rgb.float().double(), rgb.double())), "a target is no fp32 value"
    assert bool(torch.equal(torch.round(mk), mk)) and float(mk.abs().max()) <= 2, "rgb: a target is off the quantum grid"
    _budget("loss", (p["d"] ** 2).sum().reshape(1), p["d"] ** 2, 9.0 / 256.0, spans)
    qd = 1.0 / (32.0 * n)                                            # quantum of dO = m_k / (32 n)
    _budget("b2", p["do"].abs().sum(0), p["do"], qd, spans, prefill)
    t = p["do"][:, :, None] * p["h"][:, None, :]
    _budget("w2", t.abs().sum(0), t, qd * q, spans, prefill)
    _budget("dh", p["do"].abs() @ fld["w2"].double().abs(), p["dh"], qd, spans)
    _budget("b1", p["dh"].abs().sum(0), p["dh"], qd, spans, prefill)
    t = p["dh"][:, :, None] * p["x"][:, None, :L2]
    _budget("w1", t.abs().sum(0), t, qd * q, spans, prefill)
    _budget("dfeat", p["dh"].abs() @ fld["w1"].double().abs()[:, :L2], p["dfeat"], qd, spans)
    acc = torch.zeros(fld["table"].shape, dtype=F64)
    terms = [torch.zeros(0, dtype=F64)]
    for l in range(fld["active"]):
        w, rows = corners[l]
        t = w[:, :, None] * p["dfeat"][:, None, 2 * l:2 * l + 2]
        acc.index_add_(0, rows.reshape(-1), t.abs().reshape(-1, 2))
        terms.append(t.reshape(-1))
    _budget("table", acc, torch.cat(terms), qd * q, spans, prefill)
    return spans


def exact_case(resolutions, active, bitwidth, hidden, n, seed=0, coord_dim=2):
    """dict(field, coords, rgb, spans, want, unread).  Asserted here: the case is exact (check_exact); from n = 64 on the relu is hit
    on both sides, every paired level has non-zero table gradients and several samples add to the same table row; an active level
    without a twin is unread - its gradient is exactly zero."""
    fld = exact_field(resolutions, active, bitwidth, hidden, seed=seed + 13 * hidden, coord_dim=coord_dim)
    coords = exact_points(n, resolutions, seed=seed + n)
    rgb = exact_targets(n, seed=seed + 3 * n)
    spans = check_exact(fld, coords, rgb)
    want = step_reference(fld, coords, rgb)
    pairs = twin_pairs(fld)
    paired = {l for pr in pairs for l in pr}
    unread = [l for l in range(fld["active"]) if l not in paired]
    begin = fld["begin"]
    for l in unread + list(range(fld["active"], len(resolutions))):
        assert bool((want["table"][int(begin[l]):int(begin[l + 1])] == 0).all()), f"level {l} must receive nothing"
    if n >= 64 and pairs and hidden >= 16:
        p = decoder_parts(fld, coords, rgb)
        assert bool((p["a"] > 0).any()) and bool((p["a"] <= 0).any()), "the relu is hit on one side only"
        used = {l for l in paired if bool((fld["w1"][:, 2 * l:2 * l + 2] != 0).any())}
        for l in used:
            assert bool((want["table"][int(begin[l]):int(begin[l + 1])] != 0).any()), f"level {l} receives no gradient"
        count = torch.zeros(fld["table"].shape[0])
        corners = level_corners(fld, coords)
        for l in used:
            w, rows = corners[l]
            count.index_add_(0, rows.reshape(-1), (w.reshape(-1) != 0).float())
        assert int((count >= 2).sum()) >= 4, "no table row is shared by several samples"
    return dict(field=fld, coords=coords, rgb=rgb, spans=spans, want=want, unread=unread)


# the reference case: two dense levels, two hashed levels and a dead finest one
CHECKED = dict(resolutions=(8, 8, 32, 32, 64), active=4, bitwidth=8, hidden=64)
EIGHT_PAIRS = tuple(r for k in range(2, 10) for r in (2 ** k, 2 ** k))       # 4, 4, 8, 8, ..., 512, 512
# (resolutions, active, bitwidth, hidden)
EXACT_FIELDS = [(CHECKED["resolutions"], 4, 8, 64), ((4, 4), 2, 6, 2), (EIGHT_PAIRS, 16, 10, 128), (EIGHT_PAIRS, 15, 10, 128),
                (CHECKED["resolutions"], 4, 8, 34)]
EXACT_N = (1, 64, 1024)
