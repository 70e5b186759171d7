"""numpy float32 restatements of the two sums of csrc/step_tail_dev.h, addition by addition in the kernels' order.  They are the
oracle of tests/test_gpu_step_tail.py (not the kernels themselves); tests/test_step_tail_host.py checks them against float64.
Test infrastructure only."""
import numpy as np

# csrc/nerf_mlp_shape.h (hidden 64, 32 grid features, 4 view octaves)
IN, H, X2 = 32, 64, 42
NPARAM = H * IN + H + 16 * H + 16 + H * X2 + H + H * H + H + 3 * H + 3
NPARAM_PAD = (NPARAM + 63) // 64 * 64
assert NPARAM == 10259 and NPARAM_PAD == 10304


def packed_index(in_dim):
    """canonical parameter index -> index in the packed buffer (W1 in_dim wide), -1 for a padding column of W1"""
    j = np.arange(NPARAM)
    r, c = j // IN, j % IN
    w1 = np.where(c < in_dim, r * in_dim + c, -1)
    return np.where(j < H * IN, w1, j - H * (IN - in_dim))


def dw_reduce(partials, rows, in_dim, grad_params):
    """partials f32 [>= rows, NPARAM_PAD]; grad_params f32 [packed count] -> the new grad_params.
    Per element: 16 row-strided partial sums (rows ty, ty + 16, ... in order), the 16 in index order, then `+=`."""
    p = np.asarray(partials, dtype=np.float32).reshape(-1, NPARAM_PAD)[:rows, :NPARAM]
    group = np.zeros((16, NPARAM), dtype=np.float32)
    for r in range(rows):
        group[r % 16] = group[r % 16] + p[r]
    t = np.zeros(NPARAM, dtype=np.float32)
    for k in range(16):
        t = t + group[k]
    out = np.array(grad_params, dtype=np.float32, copy=True)
    dst = packed_index(in_dim)
    keep = dst >= 0
    out[dst[keep]] = out[dst[keep]] + t[keep]
    return out


def loss_sum(partial, inv_n):
    """partial f32 [n] -> f32 loss.  Thread tid of 1024 adds partial[base + tid + k * 1024], k = 0..7, block of 8192 after block; the
    64 lanes of a wave fold by shuffle-down (offsets 32 .. 1: lane l takes l + off); lane 0 of the 16 waves in index order; x inv_n."""
    x = np.asarray(partial, dtype=np.float32).reshape(-1)
    n = x.shape[0]
    pad = np.zeros((n + 8191) // 8192 * 8192 if n else 0, dtype=np.float32)
    pad[:n] = x
    t = np.zeros(1024, dtype=np.float32)
    for block in pad.reshape(-1, 8, 1024):
        for k in range(8):
            t = t + block[k]
    t = t.reshape(16, 64).copy()
    off = 32
    while off > 0:
        t[:, :64 - off] = t[:, :64 - off] + t[:, off:]
        off >>= 1
    s = np.float32(0.0)
    for w in range(16):
        s = np.float32(s + t[w, 0])
    return np.float32(s * np.float32(inv_n))
