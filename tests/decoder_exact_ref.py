"""Exact-arithmetic inputs and a plain float64 reference for the fused NeRF decoder kernels (csrc/nerf_mlp.hip,
csrc/nerf_mlp_bf16.hip, csrc/nerf_mlp_wide.hip).  Test infrastructure only.

The technique: choose inputs for which EVERY value a kernel ever rounds is exactly representable - integer features,
weights in {-1, 0, +1}, small integer biases, view direction 0 (embedding exactly 0 / 1), integer upstream gradients.  Then
the result does not depend on the summation order, on MFMA accumulation, on FMA contraction or on the bf16 packing, and a
kernel must equal the float64 restatement below BIT FOR BIT.  The one inexact function left is the sigmoid; the `paired`
mode (make_params) removes it from the backward pass: z = 0 exactly, so rgb = 1/2 and dY5 = grad_rgb / 4.

Measured on the host at S = 5003, in_dim 32, over all patterns: every intermediate <= 50 in magnitude, sum |dY||X| <= 1.0e5;
units both active and idle over the samples: h1 1.0, h2 / h3 >= 0.82 (paired) and >= 0.91 (general); in general mode >= 0.44
of the |z| are <= 4 (hidden 64: 0.60).  Weights ever non-zero: all of them over both modes; in the paired mode alone 74 % of W4,
93 % of W3, 84 % of W2 (a mirrored row repeats its partner's columns).  Gradient elements ever non-zero: all but the dW3 columns of
the embedding's input and sine columns (exactly 0 at direction 0).

`reference` applies no rounding emulation.  It ASSERTS the exactness conditions itself: a failing assertion here means the
inputs are bad, not that a kernel is wrong.
"""
import math

import torch

NF = 4                    # view-direction octaves
PE = 3 + 6 * NF           # 27
X2 = 15 + PE              # 42 inputs of the colour MLP
CHUNK = 1 << 21           # samples per scratch chunk of the hidden-128 backward (WIDE_CHUNK_SAMPLES)
MODES = ("general", "paired")


def layer_shapes(hidden, in_dim):
    """packed order of csrc/nerf_mlp_shape.h: W1 b1 W2 b2 W3 b3 W4 b4 W5 b5 (nn.Module order of nerf.py:151-173)"""
    H = hidden
    return ((H, in_dim), (H,), (16, H), (16,), (H, X2), (H,), (H, H), (H,), (3, H), (3,))


NAMES = ("W1", "b1", "W2", "b2", "W3", "b3", "W4", "b4", "W5", "b5")


def param_count(hidden, in_dim):
    return sum(math.prod(s) for s in layer_shapes(hidden, in_dim))


def unpack(params, hidden, in_dim):
    out, off = {}, 0
    for name, shp in zip(NAMES, layer_shapes(hidden, in_dim)):
        n = math.prod(shp)
        out[name] = params[off:off + n].reshape(shp)
        off += n
    assert off == params.numel()
    return out


def pack(tensors):
    return torch.cat([tensors[n].reshape(-1) for n in NAMES])


def locate(index, hidden, in_dim):
    """(layer name, row, column) of a packed parameter index - for reading a bitwise mismatch"""
    off = 0
    for name, shp in zip(NAMES, layer_shapes(hidden, in_dim)):
        n = math.prod(shp)
        if index < off + n:
            i = index - off
            return (name, i // shp[1], i % shp[1]) if len(shp) == 2 else (name, i, 0)
        off += n
    raise IndexError(index)


def embed(dirs):
    """PositionalEmbedder.forward: [d ; sin(2^k d) frequency-major axis-minor ; cos(same)] (pinned against
    oracle.nerf.positional_embed by the host test)"""
    bands = 2.0 ** torch.arange(NF, dtype=dirs.dtype, device=dirs.device)
    winded = (dirs[:, None, :] * bands[None, :, None]).reshape(dirs.shape[0], 3 * NF)
    return torch.cat([dirs, torch.sin(winded), torch.cos(winded)], dim=-1)


def _exact_in(t, dtype):
    return bool(torch.equal(t.to(dtype).to(t.dtype), t))


def reference(params, feats, dirs, grad_rgb, grad_density, hidden, io_dtypes=(torch.bfloat16, torch.float16), check=True):
    """The decoder of nerf.py:245-264 and its backward pass in float64, on the device of the inputs.
    Returns dict(rgb, density, z, grad_feats, grad_params [packed], stats)."""
    f64 = torch.float64
    in_dim = feats.shape[1]
    P = unpack(params.to(f64), hidden, in_dim)
    x = feats.to(f64)
    gr, gd = grad_rgb.to(f64), grad_density.to(f64).reshape(-1, 1)
    h1 = torch.relu(x @ P["W1"].T + P["b1"])
    y = h1 @ P["W2"].T + P["b2"]
    density = torch.relu(y[:, 0:1])
    emb = embed(dirs.to(f64))
    x2 = torch.cat([y[:, 1:], emb], dim=-1)
    h2 = torch.relu(x2 @ P["W3"].T + P["b3"])
    h3 = torch.relu(h2 @ P["W4"].T + P["b4"])
    z = h3 @ P["W5"].T + P["b5"]
    rgb = torch.sigmoid(z)

    dY5 = gr * rgb * (1.0 - rgb)
    dH3 = (dY5 @ P["W5"]) * (h3 > 0)
    dH2 = (dH3 @ P["W4"]) * (h2 > 0)
    dX2 = dH2 @ P["W3"]
    dY2 = torch.cat([gd * (y[:, 0:1] > 0), dX2[:, :15]], dim=-1)
    dH1 = (dY2 @ P["W2"]) * (h1 > 0)
    grad_feats = dH1 @ P["W1"]
    pairs = (("W5", dY5, h3), ("W4", dH3, h2), ("W3", dH2, x2), ("W2", dY2, h1), ("W1", dH1, x))
    grads = {}
    for name, dY, X in pairs:
        grads[name] = dY.T @ X
        grads["b" + name[1]] = dY.sum(0)
    stats = {}
    if check:
        bf = torch.bfloat16
        fwd = dict(feats=x, h1=h1, y_1_16=y[:, 1:], embedding=emb, b3=P["b3"], h2=h2, h3=h3)
        bwd = dict(dY5=dY5, dH3=dH3, dH2=dH2, dY2=dY2, dH1=dH1)
        for name, t in {**fwd, **bwd}.items():
            assert _exact_in(t, bf), f"inputs are not exact: {name} changes in a round trip through bf16"
        for name, t in (("weights", params.to(f64)), ("y0", y[:, 0:1]), ("grad_rgb", gr), ("grad_density", gd)):
            assert _exact_in(t, torch.float32), f"inputs are not exact: {name} is not an fp32 value"
        for dt in io_dtypes:
            assert _exact_in(x, dt), f"inputs are not exact: feats changes in a round trip through {dt}"
            assert _exact_in(grad_feats, dt), f"inputs are not exact: grad_feats changes in a round trip through {dt}"
        # weight gradients: every operand sits on the integer grid (spacing 1), and no partial sum of |dY| |X| in ANY order
        # can reach 2^24 spacings - so fp32 accumulation is exact whatever the order
        worst = 0.0
        for name, dY, X in pairs:
            assert bool((dY == dY.round()).all()) and bool((X == X.round()).all()), f"{name}: operands off the integer grid"
            worst = max(worst, float((dY.abs().T @ X.abs()).max()), float(dY.abs().sum(0).max()))
        assert worst < 2.0 ** 24, f"inputs are not exact: sum |dY||X| = {worst} reaches 2^24"
        stats = dict(max_abs=max(float(t.abs().max()) if t.numel() else 0.0 for t in list(fwd.values()) + list(bwd.values())),
                     max_sum_dy_x=worst,
                     both={k: float((((t > 0).any(0)) & ((t <= 0).any(0))).double().mean()) if t.shape[0] else 0.0
                           for k, t in (("h1", h1), ("h2", h2), ("h3", h3))},
                     z_small=float((z.abs() <= 4).double().mean()) if z.numel() else 0.0,
                     density_active=float((density > 0).double().mean()) if z.numel() else 0.0)
    return dict(rgb=rgb, density=density, z=z, grad_feats=grad_feats, grad_params=pack(grads), stats=stats)


# ---------------------------------------------------------------------------------------------------- generator
def num_patterns(hidden):
    """with three non-zeros per row, ceil(hidden / 3) patterns touch every column of the widest rows (22 / 43)"""
    return (hidden + 2) // 3


def _sparse(rows, cols, pattern, salt, row_ids=None, nnz=3, col0=0, out=None, col_ids=None):
    """[rows, cols] with min(nnz, cols) entries +-1 per row (signs mixed inside a row); the non-zero columns of row r are
    col0 + (7 r + salt + nnz pattern + j) mod cols, j < nnz: over ceil(cols / nnz) consecutive patterns they sweep the
    whole row.  `out`: write into columns col0 .. col0 + cols of an existing matrix.  `row_ids` / `col_ids` replace r in the
    signs / in the columns (rows that share both are equal)."""
    r = torch.arange(rows) if row_ids is None else row_ids
    W = torch.zeros(r.shape[0], cols, dtype=torch.float64) if out is None else out
    idx = torch.arange(r.shape[0])
    nnz = min(nnz, cols)
    for j in range(nnz):
        c = col0 + (7 * (r if col_ids is None else col_ids) + salt + nnz * pattern + j) % cols
        s = 1.0 - 2.0 * ((r + pattern + salt) % 2).double()
        if j % 3 == 1:
            s = -s
        if j % 3 == 2:
            s = 1.0 - 2.0 * (((r * 5 + pattern + salt) % 7) % 2).double()
        W[idx, c] = s
    return W


def _small_ints(n, lo, hi, pattern, salt, ids=None):
    """integers in [lo, hi], every position non-zero for some pattern"""
    r = torch.arange(n) if ids is None else ids
    return (lo + (r * 3 + pattern * 7 + salt) % (hi - lo + 1)).double()


def pairing(n, pattern, distances=(8, 16, 32)):
    """(partner, first): an involution on n units.  Units a and partner[a] = a +- d form a pair, d taken from `distances`
    (those with 2 d <= n) by the pattern; first[a] marks the lower member; the units of an incomplete last group of 2 d are
    their own partner.  The distances are wider than a row's run of non-zero columns, so that a row never reads both members
    of a pair (their equal values would cancel under the row's mixed signs)."""
    a = torch.arange(n)
    ds = [d for d in distances if 2 * d <= n]
    if not ds:
        return a, torch.zeros(n, dtype=torch.bool)
    d = ds[pattern % len(ds)]
    first = (a // d) % 2 == 0
    partner = torch.where(first, a + d, a - d)
    whole = (a // (2 * d) + 1) * 2 * d <= n
    return torch.where(whole, partner, a), first & whole


def pairing_odd(n, pattern):
    """an involution on an odd number of units: unit u = pattern mod n is its own partner - a different one from pattern to
    pattern, so that every unit is paired in most patterns - and the others, in rotating order, pair at distance (n - 1) / 2"""
    u, half = pattern % n, (n - 1) // 2
    rest = [(u + 1 + (i + pattern // n) % (n - 1)) % n for i in range(n - 1)]
    partner = torch.arange(n)
    for i in range(half):
        a, b = rest[i], rest[i + half]
        partner[a], partner[b] = b, a
    return partner


def mirror_maps(hidden, in_dim, pattern):
    """the involutions of the `paired` mode on the columns of feats, h1, y[1:16], h2 and h3"""
    return dict(x=pairing(in_dim, pattern, (8, 16, 4) if in_dim >= 8 else (2, 1))[0], h1=pairing(hidden, pattern + 1)[0],
                y=pairing_odd(15, pattern), h2=pairing(hidden, pattern)[0], h3=pairing(hidden, pattern + 1)[0])


def _mirror(W, b, q_out, q_in):
    """make row q_out(r) the row r read through q_in: W[q(r), q_in(c)] = W[r, c], equal biases.  With inputs that are
    symmetric under q_in the outputs are symmetric under q_out."""
    second = torch.arange(W.shape[0]) > q_out
    W[second] = W[q_out[second]][:, q_in]
    b[second] = b[q_out[second]]


def make_params(hidden, in_dim, pattern, mode, b2_cancel=False):
    """Packed float64 parameters (integer valued) of pattern `pattern`.

    general: any z (use with grad_rgb = 0).
    paired: the network is its own mirror image - every layer's units come in pairs (a, q(a)) whose rows read mirrored
    columns of the layer below (down to pairs of equal feature columns), so paired units carry equal values; W5 has +t on a and
    -t on q(a) and b5 = 0.  Then z = 0 exactly for every sample while no weight is zero on purpose: rgb = 1/2, dY5 =
    grad_rgb / 4, and the gradient of every layer of the colour chain is non-zero (antisymmetric under q, so it does not
    cancel on the way down as it would if the paired rows read the SAME columns)."""
    assert mode in MODES
    H = hidden
    T = dict(W1=_sparse(H, in_dim, pattern, 0), b1=_small_ints(H, -1, 2, pattern, 1),
             W2=_sparse(16, H, pattern, 2), b2=_small_ints(16, -2, 2, pattern, 3),
             W3=_sparse(H, 15, pattern, 4, nnz=2), b3=_small_ints(H, -2, 1, pattern, 5))
    # a colour row reads two geometry features and two embedding columns (a row of embedding columns alone is a constant)
    T["W3"] = _sparse(H, PE, pattern, 10, nnz=2, col0=15, out=torch.cat([T["W3"], torch.zeros(H, PE, dtype=torch.float64)], 1))
    T["b2"][0] = 2.0 + pattern % 3            # the density pre-activation: positive on a zero feature row (dead tail lanes)
    if b2_cancel:
        # the geometry features y[1:16] get a pre-bias value of 256 + (odd) that bf16 cannot hold, and a bias of -256 that
        # brings it back: exact only if b2 is added BEFORE the value is packed to bf16.  (Unit u and its mirror unit are both
        # the constant 256, so the mirrored rows below may read either.)
        u = pattern % H
        for v in (u, int(pairing(H, pattern + 1)[0][u])):
            T["W1"][v] = 0.0
            T["b1"][v] = 256.0
            T["W2"][1:, v] = 0.0
        T["W2"][1:, u] = 1.0
        T["b2"][1:] -= 256.0
    if mode == "general":
        T["W4"] = _sparse(H, H, pattern, 6)
        T["b4"] = _small_ints(H, -3 * (H // 64), 0, pattern, 7)
        T["W5"] = _sparse(3, H, pattern, 8, nnz=2)             # few entries keep |z| small; the paired W5 is dense
        T["b5"] = _small_ints(3, -1, 1, pattern, 9)
    else:
        q = mirror_maps(H, in_dim, pattern)
        T["W4"] = _sparse(H, H, pattern, 6)
        T["b4"] = _small_ints(H, -2, 1, pattern, 7)
        _mirror(T["W1"], T["b1"], q["h1"], q["x"])
        _mirror(T["W2"][1:], T["b2"][1:], q["y"], q["h1"])
        _mirror(T["W3"], T["b3"], q["h2"], torch.cat([q["y"], 15 + torch.arange(PE)]))
        _mirror(T["W4"], T["b4"], q["h3"], q["h2"])
        partner, first = pairing(H, pattern + 1)
        key = torch.minimum(torch.arange(H), partner)
        sign = torch.where(first, 1.0, -1.0).double() * (partner != torch.arange(H))
        c = torch.arange(3)[:, None]
        t = ((key[None, :] + c + pattern) % 3 - 1).double()         # -1, 0, +1 per (channel, pair)
        t = torch.where(t == 0, ((key[None, :] // 3 + c + pattern) % 2).double(), t)      # fewer zeros
        T["W5"] = t * sign[None, :]
        T["b5"] = torch.zeros(3, dtype=torch.float64)
    return pack(T)


def active_samples(S, generator, budget=4000):
    """mask of the samples that get an upstream gradient: all of them up to 5003, else about `budget` random ones plus the
    first and the last 32-sample tile of every scratch chunk (so that sum |dY||X| stays below 2^24)"""
    if S <= 5003:
        return torch.ones(S, dtype=torch.bool)
    m = torch.zeros(S, dtype=torch.bool)
    m[torch.randint(0, S, (budget,), generator=generator)] = True
    for c0 in range(0, S, CHUNK):
        c1 = min(S, c0 + CHUNK)
        m[c0:c0 + 32] = True
        m[max(c0, (c1 - 1) // 32 * 32 - 32):c1] = True
    return m


def make_case(hidden, in_dim, S, pattern, mode, b2_cancel=False):
    """Inputs of one exact case on the CPU: dict(params f32 [packed], feats f32 [S, in_dim] in {-2..2}, dirs f32 zeros,
    grad_rgb f32 (multiples of 4; zero in general mode), grad_density f32 (small integers))."""
    g = torch.Generator().manual_seed(1000 * pattern + 17 * in_dim + hidden + (S % 9973))
    feats = torch.randint(-2, 3, (S, in_dim), generator=g, dtype=torch.int8).float()
    if mode == "paired":                      # equal feature columns under the mirror map
        q = mirror_maps(hidden, in_dim, pattern)["x"]
        second = torch.arange(in_dim) > q
        feats[:, second] = feats[:, q[second]]
    act = active_samples(S, g)
    gd = torch.randint(-2, 3, (S, 1), generator=g, dtype=torch.int8).float() * act[:, None]
    if mode == "paired":
        gr = 4.0 * torch.randint(-1, 2, (S, 3), generator=g, dtype=torch.int8).float() * act[:, None]
    else:
        gr = torch.zeros(S, 3)
    return dict(params=make_params(hidden, in_dim, pattern, mode, b2_cancel).float(), feats=feats, dirs=torch.zeros(S, 3),
                grad_rgb=gr, grad_density=gd, hidden=hidden, in_dim=in_dim, S=S, pattern=pattern, mode=mode)


def run_reference(case, device=None, **kw):
    dev = device or case["feats"].device
    return reference(case["params"].to(dev), case["feats"].to(dev), case["dirs"].to(dev), case["grad_rgb"].to(dev),
                     case["grad_density"].to(dev), case["hidden"], **kw)


# ---------------------------------------------------------------------------------------------------- the cases of the GPU file
S_MAIN = 5003             # ragged: 156 full tiles + 11 samples
S_WIDTHS = 1029           # narrow-row cases: several workgroups, ragged tail
S_CANCEL = 1001           # b2_cancel case: dW2 sums 256 |dY2| per sample, kept well below 2^24
SHAPE_PATTERN = 4
SHAPE_S = (1, 31, 32, 33, 129, 70001)
WIDTHS = (1, 5, 12, 31, 32)
WIDTH_PATTERN = 5
S_TWO_CHUNKS = CHUNK + 33
HIDDENS = (64, 128)


def gpu_cases():
    """every (hidden, in_dim, S, pattern, mode, b2_cancel) the GPU file runs"""
    out = []
    for hidden in HIDDENS:
        for mode in MODES:
            out += [(hidden, 32, S_MAIN, p, mode, False) for p in range(num_patterns(hidden))]
            out += [(hidden, 32, S, SHAPE_PATTERN, mode, False) for S in SHAPE_S]
            out += [(hidden, w, S_WIDTHS, WIDTH_PATTERN, mode, False) for w in WIDTHS]
        out.append((hidden, 32, S_CANCEL, SHAPE_PATTERN, "paired", True))
    out.append((128, 32, S_TWO_CHUNKS, SHAPE_PATTERN, "paired", False))
    return out
