"""Test infrastructure: numpy restatement of SPC rendering - the first cell every ray hits (the first nugget per ray of
oracle.spc.raytrace through mark_pack_boundaries), SPCField's three colour sources and rgba, and the four buffers
PackedSPCTracer returns (wisp/models/nefs/spc_field.py:79-147, wisp/tracers/packed_spc_tracer.py:50-90)."""
import numpy as np

from oracle import spc as ospc

F32 = np.float32


def first_hit(octree, points, pyramid, exsum, origins, dirs, level):
    """(pidx i32 [R], -1 = miss; depth f32 [R,1], 0 on a miss; hit bool [R])."""
    o = np.asarray(origins, dtype=F32).reshape(-1, 3)
    R = o.shape[0]
    pidx = np.full(R, -1, dtype=np.int32)
    depth = np.zeros((R, 1), dtype=F32)
    hit = np.zeros(R, dtype=bool)
    if R:
        ridx, pid, dep = ospc.raytrace(octree, points, pyramid, exsum, o, dirs, level)
        first = ospc.mark_pack_boundaries(ridx)
        rays = ridx[first].astype(np.int64)
        pidx[rays] = pid[first]
        depth[rays] = dep[first]
        hit[rays] = True
    return pidx, depth, hit


def first_cell_per_level(octree, points, pyramid, exsum, origins, dirs, level):
    """i32 [level + 1, R]: the first cell of every level 0..level each ray hits (-1 = none)."""
    return np.stack([first_hit(octree, points, pyramid, exsum, origins, dirs, l)[0] for l in range(level + 1)])


def traversal_stats(octree, points, pyramid, exsum, origins, dirs, level):
    """dict(hitting, backtrack, enter_and_miss): rays with a first leaf; those of them whose first leaf has, at some level, an
    ancestor that is NOT the first cell of that level the ray hits (a first-hit walk has to back up for them); rays that hit a
    child of the root but no leaf (they walk into the tree and exhaust it)."""
    first = first_cell_per_level(octree, points, pyramid, exsum, origins, dirs, level)
    leaf = first[level]
    hitting = leaf >= 0
    back = np.zeros(leaf.shape[0], dtype=bool)
    for l in range(1, level):
        anc = points[np.where(hitting, leaf, 0)].astype(np.int64) >> (level - l)
        got = points[np.where(first[l] >= 0, first[l], 0)].astype(np.int64)
        back |= hitting & np.any(anc != got, axis=1)
    enter = (first[1] >= 0) & ~hitting if level >= 1 else np.zeros_like(hitting)
    return dict(hitting=int(hitting.sum()), backtrack=int(back.sum()), enter_and_miss=int(enter.sum()))


def field_colors(octree, colors=None, normals=None):
    """SPCField.colors, f32 [cells of the finest level, 4 | 3]: u8 RGBA / 255; else 0.5 * (normals + 1); else the finest level's
    cell coordinates / 2^level."""
    if colors is not None:
        return np.asarray(colors).reshape(-1, 4).astype(F32) / F32(255.0)
    if normals is not None:
        return (F32(0.5) * (np.asarray(normals, dtype=F32).reshape(-1, 3) + F32(1.0))).astype(F32)
    points, pyramid, _ = ospc.octree_to_spc(octree)
    level = pyramid.shape[1] - 2
    return points[int(pyramid[1, level]):].astype(F32) / F32(2 ** level)


def rgba(colors, pyramid, ridx_hit):
    """SPCField.rgba: f32 [batch, 1, 3] of point-hierarchy indices of the finest level."""
    level = pyramid.shape[1] - 2
    return colors[np.asarray(ridx_hit, dtype=np.int64) - int(pyramid[1, level]), :3][:, None, :]


def trace(octree, colors, origins, dirs):
    """PackedSPCTracer.trace at the finest level: dict(depth f32 [R,1], hit bool [R], rgb f32 [R,3], alpha f32 [R,1])."""
    points, pyramid, exsum = ospc.octree_to_spc(octree)
    level = pyramid.shape[1] - 2
    pidx, depth, hit = first_hit(octree, points, pyramid, exsum, origins, dirs, level)
    rgb = np.zeros((pidx.shape[0], 3), dtype=F32)
    rgb[hit] = rgba(colors, pyramid, pidx[hit])[:, 0]
    return dict(depth=depth, hit=hit, rgb=rgb, alpha=hit.astype(F32)[:, None], pidx=pidx)
