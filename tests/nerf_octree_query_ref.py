"""A float64 restatement of the radiance-field query over an octree grid (test infrastructure; the subject is
csrc/nerf_octree_query.hip): the walk of oracle/spc.py, the trilinear blend of every level, the level sum or the 'cat' row, and the
decoder of NeuralRadianceField.rgba (wisp/models/nefs/nerf.py:219-264), everything after the float32 cell arithmetic in float64.
Used for error bounds only: it says how far two float32 evaluations are from the exact value, not what their bits are."""
import numpy as np
import torch

from oracle import spc as ospc


def tree_of(grid):
    """the numpy arrays of a grid's octree and of its dual"""
    blas = grid.blas
    return dict(octree=blas.octree.detach().cpu().numpy(), exsum=blas.prefix.detach().cpu().numpy().astype(np.int64),
                points=blas.points.detach().cpu().numpy().astype(np.int64), trinkets=grid.trinkets.detach().cpu().numpy().astype(np.int64))


def chain_of(tree, coords, level):
    """int64 [n, level + 1]: the cell of every level from the root down, -1 outside the cube and from the first unoccupied child on"""
    return ospc.query(tree["octree"], tree["exsum"], np.asarray(coords, dtype=np.float32), level, with_parents=True)


def weights64(coords, pts, level):
    """the eight trilinear weights, j = dx << 2 | dy << 1 | dz; the position inside the cell is exact in float64"""
    x = (2.0 ** level) * (0.5 * coords.astype(np.float64) + 0.5) - pts.astype(np.float64)
    g = 1.0 - x
    return np.stack([(x[:, 0] if j & 4 else g[:, 0]) * (x[:, 1] if j & 2 else g[:, 1]) * (x[:, 2] if j & 1 else g[:, 2])
                     for j in range(8)], -1)


def features64(tree, tables, levels, coords, half_round=False, sum_lods=True):
    """tables: one [rows, F] array per level (the values the kernel reads: already rounded to their storage dtype).  half_round
    rounds the features and every level's result through fp16, as the lookup does.  -> float64 [n, F] or [n, L * F]"""
    coords = np.asarray(coords, dtype=np.float32)
    chain = chain_of(tree, coords, levels[-1])
    outs = []
    for table, level in zip(tables, levels):
        t = np.asarray(table, dtype=np.float64)
        if half_round:
            t = t.astype(np.float16).astype(np.float64)
        p = chain[:, level]
        ok = p >= 0
        safe = np.where(ok, p, 0)
        w = weights64(coords, tree["points"][safe], level)
        acc = (t[tree["trinkets"][safe]] * w[..., None]).sum(1) * ok[:, None]
        if half_round:
            acc = acc.astype(np.float16).astype(np.float64)
        outs.append(acc)
    return sum(outs[1:], outs[0]) if sum_lods else np.concatenate(outs, -1)


def decoder_params(nef):
    """the ten decoder tensors as float64 arrays, an absent bias as zeros"""
    dd, dc = nef.decoder_density, nef.decoder_color
    out = []
    for layer in (dd.layers[0], dd.lout, dc.layers[0], dc.layers[1], dc.lout):
        w = layer.weight.detach().cpu().double().numpy()
        b = layer.bias.detach().cpu().double().numpy() if layer.bias is not None else np.zeros(w.shape[0])
        out.append((w, b))
    return out


def view_code64(dirs, freqs=4):
    d = np.asarray(dirs, dtype=np.float32).astype(np.float64)
    wound = (d[:, None, :] * (2.0 ** np.arange(freqs))[None, :, None]).reshape(d.shape[0], -1)      # frequency-major, axis-minor
    return np.concatenate([d, np.sin(wound), np.cos(wound)], -1)


def decoder64(params, feats, dirs=None):
    """(rgb [n,3] or None, density [n,1])"""
    (w1, b1), (w2, b2), (w3, b3), (w4, b4), (w5, b5) = params
    y = np.maximum(feats @ w1.T + b1, 0.0) @ w2.T + b2
    density = np.maximum(y[:, 0:1], 0.0)
    if dirs is None:
        return None, density
    x2 = np.concatenate([y[:, 1:], view_code64(dirs)], -1)
    h = np.maximum(np.maximum(x2 @ w3.T + b3, 0.0) @ w4.T + b4, 0.0)
    return 1.0 / (1.0 + np.exp(-(h @ w5.T + b5))), density


def decoded_rows(logits, dictionary):
    """CodebookOctreeGrid in eval mode: dictionary[argmax(row)], the first index on ties (np.argmax's rule)"""
    return np.asarray(dictionary)[np.argmax(np.asarray(logits), axis=-1)]


def field64(nef, coords, dirs=None, lod_idx=None):
    """(rgb, density) in float64 of an OctreeGrid / CodebookOctreeGrid (eval mode) radiance field, on the CPU"""
    from wisp.models.grids import CodebookOctreeGrid
    grid = nef.grid
    num = (grid.num_lods if lod_idx is None else lod_idx + 1)
    feats = [f.detach().float().cpu().numpy() for f in list(grid.features)[:num]]
    if isinstance(grid, CodebookOctreeGrid):
        tables, half = [decoded_rows(f, d.detach().cpu().numpy()) for f, d in zip(feats, list(grid.dictionary)[:num])], False
    else:
        tables, half = feats, bool(grid.half_features)
    x = features64(tree_of(grid), tables, [int(l) for l in grid.active_lods[:num]],
                   torch.as_tensor(coords).detach().cpu().numpy(), half_round=half, sum_lods=grid.multiscale_type == 'sum')
    d = None if dirs is None else torch.as_tensor(dirs).detach().cpu().numpy()
    return decoder64(decoder_params(nef), x, d)
