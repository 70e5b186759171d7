"""Autograd front of the fused NeRF decoder kernel (csrc/nerf_mlp.hip).

Covers NeuralRadianceField.rgba after the grid lookup (wisp/models/nefs/nerf.py:245-264): density MLP, positional
encoding of the view direction, colour MLP, relu / sigmoid.  Parameters are handed to the kernel as one packed fp32
vector in nn.Module order (W1 b1 W2 b2 W3 b3 W4 b4 W5 b5); when the trainer keeps them in one flat buffer
(wisp.trainers.FlatParams) the packed vector and its gradient are zero-copy views of that buffer.
"""
import torch

# decoder shapes the kernels are built for: every app/nerf config of the reference (grid feature width 32 for nerf_hash,
# 5 for nerf_octree / nerf_codebook, 12 for nerf_triplanar; hidden 64, one hidden layer, 4 view octaves)
SUPPORTED = dict(max_in_dim=32, hidden=64, view_freqs=4)
# hidden widths with a fused kernel: 64 (register-chained forward AND weight gradients, fp32 or bf16 compute) and 128 (the
# reference's best nerf_hash row / the documented VQAD command line: csrc/nerf_mlp_wide.hip, bf16 compute only)
FUSED_HIDDEN = (64, 128)
BF16_ONLY_HIDDEN = (128,)


def _compute_bf16(nef):
    mode = getattr(nef, 'decoder_compute', 'auto')
    return (mode == 'bf16') or (mode == 'auto' and torch.is_autocast_enabled())


def _hip():
    import wisp._C as _C
    return _C


def _decoder_tensors(nef):
    dd, dc = nef.decoder_density, nef.decoder_color
    layers = [dd.layers[0], dd.lout, dc.layers[0], dc.layers[1], dc.lout]
    out = []
    for l in layers:
        out.append(l.weight)
        out.append(l.bias)          # may be None (bias=False configs)
    return out


def _flat_view(tensors):
    """One contiguous fp32 view covering `tensors` if they sit back to back in the same storage, else None."""
    if any(t is None for t in tensors):
        return None
    first = tensors[0]
    ptr, total = first.data_ptr(), 0
    for t in tensors:
        if t.dtype != torch.float32 or not t.is_contiguous() or t.data_ptr() != ptr + 4 * total:
            return None
        total += t.numel()
    return torch.empty(0, dtype=torch.float32, device=first.device).set_(first.untyped_storage(), first.storage_offset(),
                                                                         (total,), (1,))


def _pack(tensors, shapes):
    parts = []
    for t, shp in zip(tensors, shapes):
        parts.append(torch.zeros(shp, dtype=torch.float32, device=tensors[0].device).reshape(-1) if t is None
                     else t.detach().reshape(-1).float())
    return torch.cat(parts)


class _FusedDecoder(torch.autograd.Function):
    @staticmethod
    def forward(ctx, feats, dirs, compute_bf16, shapes, *params):
        C = _hip()
        flat = _flat_view([p.detach() if p is not None else None for p in params])
        packed = flat if flat is not None else _pack(params, shapes)
        hidden = shapes[0][0]
        rgb, density = C.nerf_mlp_forward(feats.detach(), dirs, packed, feats.shape[-1], hidden, SUPPORTED["view_freqs"],
                                          compute_bf16)
        ctx.save_for_backward(feats.detach(), dirs, packed)
        ctx.compute_bf16, ctx.shapes = compute_bf16, shapes
        # in-place gradient accumulation when the parameters' .grad tensors are views of one flat buffer
        grads = [getattr(p, 'grad', None) if p is not None else None for p in params]
        ctx.grad_flat = _flat_view(grads) if (flat is not None and all(g is not None for g in grads)) else None
        ctx.present = [p is not None for p in params]
        return rgb, density

    @staticmethod
    def backward(ctx, g_rgb, g_density):
        C = _hip()
        feats, dirs, packed = ctx.saved_tensors
        if g_rgb is None:
            g_rgb = torch.zeros(feats.shape[0], 3, device=feats.device)
        if g_density is None:
            g_density = torch.zeros(feats.shape[0], 1, device=feats.device)
        g_feats, g_params = C.nerf_mlp_backward(feats, dirs, packed, g_rgb.contiguous().float(), g_density.contiguous().float(),
                                                feats.shape[-1], ctx.shapes[0][0], SUPPORTED["view_freqs"],
                                                ctx.compute_bf16, grad_params=ctx.grad_flat)
        if ctx.grad_flat is not None:
            return (g_feats, None, None, None) + tuple(None for _ in ctx.present)
        outs, off = [], 0
        for shp, present in zip(ctx.shapes, ctx.present):
            n = 1
            for s in shp:
                n *= s
            outs.append(g_params[off:off + n].reshape(shp) if present else None)
            off += n
        return (g_feats, None, None, None) + tuple(outs)


def supports(nef, feats):
    if nef.hidden_dim not in FUSED_HIDDEN or (nef.hidden_dim in BF16_ONLY_HIDDEN and not _compute_bf16(nef)):
        return False
    return (feats.is_cuda and 1 <= feats.shape[-1] <= SUPPORTED["max_in_dim"]
            and nef.view_multires == SUPPORTED["view_freqs"] and nef.num_layers == 1 and nef.pos_embedder is None
            and nef.view_embedder_type == 'positional' and nef.activation_type == 'relu'
            and nef.layer_type in ('linear', 'none') and feats.dtype in (torch.float32, torch.float16, torch.bfloat16))


def prune_query_supported(nef):
    """The fused density query of the prune (csrc/prune_query.hip) covers this field: a CUDA 'cat' HashGrid of two-feature 3-D
    levels (at most 16) with an fp32 master table, the fused decoder at hidden 64 with fp32 compute, and dense_points holding
    every cell of the octree's finest level (what BLAS.from_leaf_mask needs).  WISP_PRUNE_FUSED=0 switches it off."""
    import os
    from wisp.models.grids import HashGrid
    if os.environ.get("WISP_PRUNE_FUSED", "1") == "0" or not getattr(nef, 'fused_decoder', False) or torch.is_autocast_enabled():
        return False
    grid = nef.grid
    if not isinstance(grid, HashGrid) or grid.multiscale_type != 'cat' or grid.coord_dim != 3 or grid.feature_dim != 2 \
            or not 1 <= grid.num_lods <= 16 or len(grid.active_lods) != grid.num_lods or getattr(grid, 'blas', None) is None:
        return False
    table = grid.codebook.feats
    if not table.is_cuda or table.dtype != torch.float32 or nef.hidden_dim != SUPPORTED["hidden"] or _compute_bf16(nef):
        return False
    from types import SimpleNamespace
    if not supports(nef, SimpleNamespace(is_cuda=True, shape=(0, nef.effective_feature_dim()), dtype=torch.float32)):
        return False                                       # (what the lookup would hand the decoder: fp32 rows on the table's device)
    if any(t is not None and (not t.is_cuda or t.dtype != torch.float32) for t in _decoder_tensors(nef)[:4]):
        return False
    level = grid.blas.max_level
    return (hasattr(grid.blas.__class__, "from_leaf_mask") and grid.dense_points.shape[0] == 8 ** level and level <= 9)


def fused_prune_query(nef, unit_samples, debug=False, pad_rows=0):
    """(new occupancy f32 [cells], keep bool [cells]) of NeuralRadianceField.prune for a field prune_query_supported() accepts;
    nef.grid.occupancy is the occupancy BEFORE the decay."""
    C = _hip()
    grid = nef.grid
    cb = grid.codebook
    params = _decoder_tensors(nef)
    H, I = nef.hidden_dim, nef.effective_feature_dim()
    shapes = ((H, I), (H,), (16, H), (16,), (H, 42), (H,), (H, H), (H,), (3, H), (3,))
    flat = _flat_view([p.detach() if p is not None else None for p in params])
    packed = flat if flat is not None else _pack(params, shapes)
    lod_idx = len(grid.active_lods) - 1                   # what NeuralRadianceField.rgba queries; 'cat' zeroes the columns from there on
    res = [int(r) for r in cb.resolutions.reshape(-1).tolist()]
    return C.nerf_prune_query(grid.dense_points, unit_samples, grid.blas.max_level, cb.feats.detach(), cb.begin_idxes, res,
                              grid.codebook_bitwidth, lod_idx * grid.feature_dim, packed, I, H, grid.occupancy,
                              nef.prune_density_decay, nef.prune_min_density, debug=debug, pad_rows=pad_rows)


def nerf_query_supported(nef, lod_idx=None):
    """The fused inference query (csrc/nerf_query.hip) covers this field: a CUDA 'cat' HashGrid of two-feature 3-D levels (at most
    16) with an fp32 master table, and the fused decoder at hidden 64 with fp32 compute, outside autocast, with all ten decoder
    tensors on the device in fp32 (an absent bias counts as zeros).  WISP_NERF_QUERY_FUSED=0 switches it off."""
    import os
    from wisp.models.grids import HashGrid
    if os.environ.get("WISP_NERF_QUERY_FUSED", "1") == "0" or not getattr(nef, 'fused_decoder', False) or torch.is_autocast_enabled():
        return False
    grid = nef.grid
    if not isinstance(grid, HashGrid) or grid.multiscale_type != 'cat' or grid.coord_dim != 3 or grid.feature_dim != 2 \
            or not 1 <= grid.num_lods <= 16 or len(grid.active_lods) != grid.num_lods:
        return False
    if lod_idx is not None and not 0 <= lod_idx < grid.num_lods:
        return False
    table = grid.codebook.feats
    if not table.is_cuda or table.dtype != torch.float32 or nef.hidden_dim != SUPPORTED["hidden"] or _compute_bf16(nef):
        return False
    from types import SimpleNamespace
    if not supports(nef, SimpleNamespace(is_cuda=True, shape=(0, nef.effective_feature_dim()), dtype=torch.float32)):
        return False                                       # (what the lookup would hand the decoder: fp32 rows on the table's device)
    return not any(t is not None and (not t.is_cuda or t.dtype != torch.float32) for t in _decoder_tensors(nef))


def fused_nerf_query(nef, coords, ray_d=None, ray_dirs=None, ridx=None, lod_idx=None, want_rgb=True, pad_rows=0):
    """(rgb [n,3] fp32 or None, density [n,1] fp32) of NeuralRadianceField.rgba for a field nerf_query_supported() accepts, in one
    launch and without a feature tensor; the same bits as grid.interpolate + fused_nerf_decoder.  The view direction comes per
    sample (ray_d [n,3]) or per ray (ray_dirs [R,3] with ridx int64 [n]: ray_dirs.index_select(0, ridx) is never built).
    Inference only: inputs that require a gradient are refused."""
    tensors = [coords, ray_d, ray_dirs] + [nef.grid.codebook.feats] + _decoder_tensors(nef)
    if torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in tensors):
        raise NotImplementedError("fused_nerf_query has no backward: call it under torch.no_grad(), or take the modular path")
    if (ray_d is None) == (ray_dirs is None) and want_rgb:
        raise ValueError("give the view direction either per sample (ray_d) or per ray (ray_dirs + ridx)")
    if (ray_dirs is None) != (ridx is None):
        raise ValueError("ray_dirs and ridx go together")
    C = _hip()
    grid = nef.grid
    cb = grid.codebook
    params = _decoder_tensors(nef)
    H, I = nef.hidden_dim, nef.effective_feature_dim()
    shapes = ((H, I), (H,), (16, H), (16,), (H, 42), (H,), (H, H), (H,), (3, H), (3,))
    flat = _flat_view([p.detach() if p is not None else None for p in params])
    packed = flat if flat is not None else _pack(params, shapes)
    if lod_idx is None:
        lod_idx = len(grid.active_lods) - 1               # what NeuralRadianceField.rgba queries; 'cat' zeroes the columns from there on
    res = [int(r) for r in cb.resolutions.reshape(-1).tolist()]
    rgb, density = C.nerf_query(coords.detach(), (ray_d if ray_d is not None else ray_dirs), ridx, cb.feats.detach(), cb.begin_idxes,
                                res, grid.codebook_bitwidth, lod_idx * grid.feature_dim, packed, I, H, want_rgb=want_rgb,
                                pad_rows=pad_rows)
    return rgb, density.reshape(-1, 1)


def nerf_octree_query_supported(nef, lod_idx=None):
    """The fused inference query of the octree family (csrc/nerf_octree_query.hip) covers this field: a CUDA OctreeGrid whose
    multi-level lookup is the one-launch one (`_fusable()`), or a CUDA CodebookOctreeGrid in eval mode with 2-D fp32 logits (not
    baked), an fp32 dictionary of at most 256 entries and at most 16 features; 'linear' interpolation; 'sum' at any valid
    lod_idx, or 'cat' at the last one; and the decoder conditions of nerf_query_supported.  The switch
    WISP_NERF_OCTREE_QUERY_FUSED must be set to something other than 0: its default is off, because on the nerf_octree.yaml field
    a whole view at render_batch 10 000 did not beat the modular ops outside the spread of the repetitions
    (profiles/bench_nerf_octree_eval.json)."""
    import os
    from wisp.models.grids import CodebookOctreeGrid, OctreeGrid
    if os.environ.get("WISP_NERF_OCTREE_QUERY_FUSED", "0") == "0" or not getattr(nef, 'fused_decoder', False) \
            or torch.is_autocast_enabled():
        return False
    grid = nef.grid
    if not isinstance(grid, OctreeGrid) or grid.interpolation_type != 'linear' or grid.multiscale_type not in ('cat', 'sum') \
            or not 1 <= grid.num_lods <= 16 or len(grid.active_lods) != grid.num_lods or not 1 <= grid.feature_dim <= 16:
        return False
    last = grid.num_lods - 1
    if lod_idx is None:
        lod_idx = last
    if not 0 <= lod_idx <= last or (grid.multiscale_type == 'cat' and lod_idx != last):
        return False
    if isinstance(grid, CodebookOctreeGrid):
        if grid.training or type(grid)._interpolate is not CodebookOctreeGrid._interpolate or not getattr(grid, 'fused', False):
            return False
        for logits, dictionary in zip(grid.features, grid.dictionary):
            if not logits.is_cuda or not dictionary.is_cuda or logits.ndim != 2 or logits.dtype != torch.float32 \
                    or dictionary.dtype != torch.float32 or logits.shape[1] != dictionary.shape[0] \
                    or not dictionary.shape[1] <= dictionary.shape[0] <= 256 or dictionary.shape[1] != grid.feature_dim:
                return False
    else:
        if not grid._fusable() or any(not f.is_cuda or f.dtype != grid.features[0].dtype or f.ndim != 2 for f in grid.features) \
                or grid.features[0].dtype not in (torch.float32, torch.float16, torch.bfloat16):
            return False
    if nef.hidden_dim != SUPPORTED["hidden"] or _compute_bf16(nef) or nef.effective_feature_dim() > SUPPORTED["max_in_dim"]:
        return False
    from types import SimpleNamespace
    if not supports(nef, SimpleNamespace(is_cuda=True, shape=(0, nef.effective_feature_dim()), dtype=torch.float32)):
        return False                                       # (what the lookup would hand the decoder: fp32 rows on the grid's device)
    return not any(t is not None and (not t.is_cuda or t.dtype != torch.float32) for t in _decoder_tensors(nef))


def fused_nerf_octree_query(nef, coords, ray_d=None, ray_dirs=None, ridx=None, lod_idx=None, want_rgb=True, pad_rows=0):
    """(rgb [n,3] fp32 or None, density [n,1] fp32) of NeuralRadianceField.rgba for a field nerf_octree_query_supported() accepts,
    in one launch and without a chain or a feature tensor; the same bits as grid.interpolate + fused_nerf_decoder (for a codebook
    grid's 'sum' over three or more levels: up to the order in which torch adds the levels).  A codebook grid is read through its
    decoded rows (CodebookOctreeGrid.decoded_tables).  View directions as fused_nerf_query takes them.  Inference only: inputs
    that require a gradient are refused."""
    from wisp.models.grids import CodebookOctreeGrid
    grid = nef.grid
    codebook = isinstance(grid, CodebookOctreeGrid)
    tensors = [coords, ray_d, ray_dirs] + list(grid.features) + (list(grid.dictionary) if codebook else []) + _decoder_tensors(nef)
    if torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in tensors):
        raise NotImplementedError("fused_nerf_octree_query has no backward: call it under torch.no_grad(), or take the modular path")
    if (ray_d is None) == (ray_dirs is None) and want_rgb:
        raise ValueError("give the view direction either per sample (ray_d) or per ray (ray_dirs + ridx)")
    if (ray_dirs is None) != (ridx is None):
        raise ValueError("ray_dirs and ridx go together")
    C = _hip()
    C._need(coords, torch.float32, "coords")               # a field or positions on the CPU: no fallback
    C._need(grid.features[0], None, "features")
    if lod_idx is None:
        lod_idx = len(grid.active_lods) - 1
    sum_lods = grid.multiscale_type == 'sum'
    if not 0 <= lod_idx < len(grid.active_lods) or (not sum_lods and lod_idx != len(grid.active_lods) - 1):
        raise ValueError(f"lod_idx {lod_idx}: 'sum' takes any level of the grid, 'cat' the last one")
    params = _decoder_tensors(nef)
    H, I = nef.hidden_dim, nef.effective_feature_dim()
    shapes = ((H, I), (H,), (16, H), (16,), (H, 42), (H,), (H, H), (H,), (3, H), (3,))
    flat = _flat_view([p.detach() if p is not None else None for p in params])
    packed = flat if flat is not None else _pack(params, shapes)
    num = lod_idx + 1
    grid._sync_device(coords.device)
    if codebook:
        tables, half_round = grid.decoded_tables()[:num], False
    else:
        tables, half_round = [grid.features[i].detach() for i in range(num)], bool(grid.half_features)
    trinkets = grid.trinkets if grid.trinkets.dtype == torch.int32 else grid.trinkets.int()
    rgb, density = C.nerf_octree_query(coords.detach(), (ray_d if ray_d is not None else ray_dirs), ridx, grid.blas.octree,
                                       grid.blas.prefix, grid.blas.points, trinkets.contiguous(), grid.blas.max_level, tables,
                                       [int(l) for l in grid.active_lods[:num]], half_round, sum_lods, packed, I, H,
                                       want_rgb=want_rgb, pad_rows=pad_rows)
    return rgb, density.reshape(-1, 1)


def _triplane_planes(grid, num):
    return [p for i in range(num) for p in (grid.features[i].fmx, grid.features[i].fmy, grid.features[i].fmz)]


def nerf_triplane_query_supported(nef, lod_idx=None):
    """The fused inference query of a triplanar field (csrc/nerf_triplane_query.hip) covers this field: a CUDA TriplanarGrid with
    'linear' interpolation; 'sum' at any valid lod_idx (levels 0..lod_idx), or 'cat' at the last one; f32 contiguous planes; at
    most 32 feature columns; and the decoder conditions of nerf_query_supported.  WISP_NERF_TRIPLANE_QUERY_FUSED=0 switches it off:
    the default is on, because on the nerf_triplanar.yaml field the slowest fused repetition beat the fastest modular one in every
    measured row (profiles/bench_nerf_triplanar_eval.json, fused against modular, median ms: query at 2^18 samples 0.348 against
    0.375 - slowest fused 0.3669, fastest modular 0.3671: a tie at that size - at 2^21 1.440 against 2.445, an 800 x 800 view at
    render_batch 10 000 213 against 388 and at 2^17 192 against 371)."""
    import os
    from wisp.models.grids import TriplanarGrid
    if os.environ.get("WISP_NERF_TRIPLANE_QUERY_FUSED", _TRIPLANE_QUERY_DEFAULT) == "0" or not getattr(nef, 'fused_decoder', False) \
            or torch.is_autocast_enabled():
        return False
    grid = nef.grid
    if not isinstance(grid, TriplanarGrid) or grid.interpolation_type != 'linear' or grid.multiscale_type not in ('cat', 'sum') \
            or not 1 <= grid.num_lods <= 16 or len(grid.features) != grid.num_lods or grid.feature_dim < 3 or grid.feature_dim % 3:
        return False
    last = grid.num_lods - 1
    if lod_idx is None:
        lod_idx = last
    if not 0 <= lod_idx <= last or (grid.multiscale_type == 'cat' and lod_idx != last):
        return False
    fdim = grid.feature_dim // 3
    for i, p in enumerate(_triplane_planes(grid, lod_idx + 1)):
        size = grid.features[i // 3].fsize + 1
        if not p.is_cuda or p.dtype != torch.float32 or not p.is_contiguous() or tuple(p.shape[-3:]) != (fdim, size, size) \
                or p.numel() != fdim * size * size:
            return False
    if nef.hidden_dim != SUPPORTED["hidden"] or _compute_bf16(nef) or nef.effective_feature_dim() > SUPPORTED["max_in_dim"] \
            or nef.effective_feature_dim() != (1 if grid.multiscale_type == 'sum' else grid.num_lods) * grid.feature_dim:
        return False
    from types import SimpleNamespace
    if not supports(nef, SimpleNamespace(is_cuda=True, shape=(0, nef.effective_feature_dim()), dtype=torch.float32)):
        return False                                       # (what the lookup would hand the decoder: fp32 rows on the grid's device)
    return not any(t is not None and (not t.is_cuda or t.dtype != torch.float32) for t in _decoder_tensors(nef))


# the default of WISP_NERF_TRIPLANE_QUERY_FUSED (see nerf_triplane_query_supported)
_TRIPLANE_QUERY_DEFAULT = "1"


def fused_nerf_triplane_query(nef, coords, ray_d=None, ray_dirs=None, ridx=None, lod_idx=None, want_rgb=True, pad_rows=0,
                              want_feats=False):
    """(rgb [n,3] fp32 or None, density [n,1] fp32) of NeuralRadianceField.rgba for a field nerf_triplane_query_supported() accepts,
    in one launch and without a feature tensor: the feature rows of the triplanar SDF kernels' encoder (equal to
    grid.interpolate's up to the rounding of its contracted multiply-adds) and, on those rows, the bits of fused_nerf_decoder.
    With want_feats a third result: those rows, fp32 [n, in_dim].  Nothing is cached: the planes are read through their parameters
    at every call.  View directions as fused_nerf_query takes them.  Inference only: inputs that require a gradient are refused."""
    grid = nef.grid
    tensors = [coords, ray_d, ray_dirs] + _triplane_planes(grid, len(grid.features)) + _decoder_tensors(nef)
    if torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in tensors):
        raise NotImplementedError("fused_nerf_triplane_query has no backward: call it under torch.no_grad(), or take the modular path")
    if (ray_d is None) == (ray_dirs is None) and want_rgb:
        raise ValueError("give the view direction either per sample (ray_d) or per ray (ray_dirs + ridx)")
    if (ray_dirs is None) != (ridx is None):
        raise ValueError("ray_dirs and ridx go together")
    C = _hip()
    C._need(coords, torch.float32, "coords")               # a field or positions on the CPU: no fallback
    C._need(grid.features[0].fmx, None, "planes")
    if lod_idx is None:
        lod_idx = grid.num_lods - 1
    sum_lods = grid.multiscale_type == 'sum'
    if not 0 <= lod_idx < grid.num_lods or (not sum_lods and lod_idx != grid.num_lods - 1):
        raise ValueError(f"lod_idx {lod_idx}: 'sum' takes any level of the grid, 'cat' the last one")
    params = _decoder_tensors(nef)
    H, I = nef.hidden_dim, nef.effective_feature_dim()
    shapes = ((H, I), (H,), (16, H), (16,), (H, 42), (H,), (H, H), (H,), (3, H), (3,))
    flat = _flat_view([p.detach() if p is not None else None for p in params])
    packed = flat if flat is not None else _pack(params, shapes)
    num = lod_idx + 1
    planes = [p.detach() for p in _triplane_planes(grid, num)]
    sizes = [int(grid.features[i].fsize) + 1 for i in range(num)]
    out = C.nerf_triplane_query(coords.detach(), (ray_d if ray_d is not None else ray_dirs), ridx, planes, sizes, grid.feature_dim // 3,
                                sum_lods, packed, I, H, want_rgb=want_rgb, pad_rows=pad_rows, want_feats=want_feats)
    if want_feats:
        return out[0], out[1].reshape(-1, 1), out[2]
    return out[0], out[1].reshape(-1, 1)


def fused_nerf_decoder(nef, feats, ray_d):
    """(rgb [S,3] fp32, density [S,1] fp32) for the decoder shapes of the reference's app/nerf configs (see SUPPORTED)."""
    compute_bf16 = _compute_bf16(nef)
    params = _decoder_tensors(nef)
    H, I = nef.hidden_dim, feats.shape[-1]
    shapes = ((H, I), (H,), (16, H), (16,), (H, 42), (H,), (H, H), (H,), (3, H), (3,))
    return _FusedDecoder.apply(feats.contiguous(), ray_d.contiguous().float(), compute_bf16, shapes, *params)
