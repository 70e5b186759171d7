"""compute_sdf / closest_point / closest_point_on_triangle (wisp/ops/mesh/compute_sdf.py:18-42, closest_point.py:17-127).  The
signed distances come from the brute-force HIP kernels behind wisp._C.external (csrc/mesh_sdf.hip); the closest point on the
chosen triangle is construction-time torch code."""
import torch


def _device_fp64(V, F, points):
    dev = torch.device("cuda", torch.cuda.current_device())
    V = V.to(dev, torch.float64)
    mesh = V[F.to(dev, torch.int64)].contiguous()
    return mesh, points.to(dev, torch.float64).reshape(-1, 3).contiguous()


def compute_sdf(V: torch.Tensor, F: torch.Tensor, points: torch.Tensor, split_size: int = 10 ** 6):
    """[N,1] float64 signed distances of `points` to the triangle mesh (V [#V,3], F [#F,3]) on the current device.  Inputs may
    be float32 or float64, on the host or the device: they are converted to float64 on the current device (the reference
    passes them through unconverted).  `split_size` is kept for API compatibility; how the points are chunked does not change a
    bit of the result."""
    import wisp._C as _C
    mesh, points = _device_fp64(V, F, points)
    if points.shape[0] == 0:
        return points.new_zeros(0, 1)
    sdfs = [_C.external.mesh_to_sdf_cuda(p.contiguous(), mesh)[0] for p in torch.split(points, max(int(split_size), 1))]
    return torch.cat(sdfs)[..., None]


def closest_point(V: torch.Tensor, F: torch.Tensor, points: torch.Tensor, split_size: int = 10 ** 6):
    """(signed distance f64 [N], closest point on the mesh f64 [N,3], index of the nearest triangle int64 [N]).  The nearest
    triangle is the lowest index among the triangles whose float-rounded squared distance is the minimum."""
    import wisp._C as _C
    mesh, points = _device_fp64(V, F, points)
    dists, hits, tidx = [], [], []
    for p in torch.split(points, max(int(split_size), 1)):
        out = _C.external.mesh_to_sdf_triangle_cuda(p.contiguous(), mesh)[0]
        n = p.shape[0]
        idx = out[n:].long()
        dists.append(out[:n])
        hits.append(closest_point_on_triangle(mesh.index_select(0, idx.clamp(min=0)), p))
        tidx.append(idx)
    if not dists:
        return points.new_zeros(0), points.new_zeros(0, 3), torch.zeros(0, dtype=torch.int64, device=points.device)
    return torch.cat(dists), torch.cat(hits), torch.cat(tidx)


def closest_point_on_triangle(triangles: torch.Tensor, points: torch.Tensor):
    """Closest point of triangle k ([n,3,3]) to point k ([n,3]).  The point's Voronoi region of the triangle (three vertices,
    three edges, the face) is decided from the six dot products of the edges a->b, a->c with the point's offsets from a, b and c;
    every candidate is computed for every pair and the region picks one, vertex regions first, then edges, then the face."""
    a, b, c = triangles[:, 0], triangles[:, 1], triangles[:, 2]
    ab, ac = b - a, c - a

    def dot(x, y):
        return (x * y).sum(-1)

    ap, bp, cp = points - a, points - b, points - c
    d1, d2 = dot(ab, ap), dot(ac, ap)
    d3, d4 = dot(ab, bp), dot(ac, bp)
    d5, d6 = dot(ab, cp), dot(ac, cp)
    va, vb, vc = d3 * d6 - d5 * d4, d5 * d2 - d1 * d6, d1 * d4 - d3 * d2
    # candidates (non-finite where their region does not apply; torch.where never picks those)
    on_ab = a + (d1 / (d1 - d3))[:, None] * ab
    on_ac = a + (d2 / (d2 - d6))[:, None] * ac
    w_bc = (d4 - d3) / ((d4 - d3) + (d5 - d6))
    on_bc = b + w_bc[:, None] * (c - b)
    inv = 1.0 / (va + vb + vc)
    inside = a + ab * (vb * inv)[:, None] + ac * (vc * inv)[:, None]
    regions = [((d1 <= 0) & (d2 <= 0), a),
               ((d3 >= 0) & (d4 <= d3), b),
               ((vc <= 0) & (d1 >= 0) & (d3 <= 0), on_ab),
               ((d6 >= 0) & (d5 <= d6), c),
               ((vb <= 0) & (d2 >= 0) & (d6 <= 0), on_ac),
               ((va <= 0) & ((d4 - d3) >= 0) & ((d5 - d6) >= 0), on_bc)]
    out = inside
    for cond, value in reversed(regions):                 # the first region that applies wins
        out = torch.where(cond[:, None], value, out)
    return out
