"""The textured-torus scene of tests/golden/mesh_tex_ref.npz and a torch-CPU restatement of what wisp_mesh_closest_tex /
wisp_mesh_sample_tex compute (include/wisp_hip.h spells the arithmetic out): every operation rounded on its own, sums of three
products as (p0 + p1) + p2, fp64 up to the clipped barycentric weights, fp32 behind them.  Also the reference's own closest_tex
chain executed where it lies (host tests and the fixture maker; the reference tree is not needed on a GPU machine)."""
import json
import os
import re
import types

import numpy as np
import torch

import mesh_sdf_oracle as oracle

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "mesh_tex_ref.npz")
REF = "/root/reference"
NU, NV = 12, 8
# colour bound against the reference chain: the lookup is Lipschitz in UV (constant <= (size - 1) * max texel step <= 15 per
# unit UV on maps of at most 16 texels); the UV differs by the fp32 rounding of the edge vectors' dot products (relative 6e-8 on
# weights <= 1, times UV spans <= 4) and by summation order: a few 1e-6.  1e-4 leaves more than a decade.
RGB_BOUND = 1e-4
HIT_BOUND = 1e-12
MARGINS = os.path.join(os.path.dirname(HERE), "profiles", "mesh_tex_test_margins.jsonl")


def record(test, **values):
    """Print one measured line and append it to profiles/mesh_tex_test_margins.jsonl."""
    line = dict(test=test, **{k: (float(v) if isinstance(v, (float, np.floating)) else v) for k, v in values.items()})
    print(json.dumps(line))
    try:
        with open(MARGINS, "a") as f:
            f.write(json.dumps(line) + "\n")
    except OSError:
        pass


def scene():
    """(V f64 [96,3] with fp32-representable values, F i64 [192,3], texv f32 [117,2], texf i64 [192,4], mats) - torus(12, 8) with
    per-quad UVs u = 2i/nu - 0.5, v = 4j/nv - 1 (outside [0,1] on purpose; seamless across the wrap under reflection, whose period
    is 2), material i % 3 for j < 6 and none for the rest; material 0 has a 5x9 RGB map, 1 only Kd, 2 a 16x1 RGBA map."""
    V, F = oracle.torus(nu=NU, nv=NV)
    V = V.astype(np.float32).astype(np.float64)
    texv = np.array([[2.0 * i / NU - 0.5, 4.0 * j / NV - 1.0] for i in range(NU + 1) for j in range(NV + 1)], dtype=np.float32)
    texf = []
    for i in range(NU):
        for j in range(NV):
            a, b, c, d = i * (NV + 1) + j, (i + 1) * (NV + 1) + j, (i + 1) * (NV + 1) + j + 1, i * (NV + 1) + j + 1
            m = i % 3 if j < 6 else -1
            texf += [(a, b, c, m), (a, c, d, m)]
    rng = np.random.default_rng(20)
    mats = {0: {'diffuse': torch.tensor([0.9, 0.1, 0.2]), 'diffuse_texname': torch.from_numpy(rng.random((5, 9, 3), dtype=np.float32))},
            1: {'diffuse': torch.tensor([0.25, 0.5, 0.75])},
            2: {'diffuse': torch.tensor([0.3, 0.3, 0.3]), 'diffuse_texname': torch.from_numpy(rng.random((16, 1, 4), dtype=np.float32))}}
    return V, F, texv, np.array(texf, dtype=np.int64), mats


def unique_points(V, F, n=2000, seed=21):
    """n fp32-representable points: an interior point of a random face (barycentric weights >= 0.1) moved along the normal by up
    to +-0.03 - the nearest triangle of such a point is unique, which random points in a box are not."""
    rng = np.random.default_rng(seed)
    T = V[F]
    t = rng.integers(0, F.shape[0], n)
    w = 0.1 + 0.7 * rng.dirichlet(np.ones(3), n)
    p = (T[t] * w[:, :, None]).sum(1)
    nrm = np.cross(T[t, 1] - T[t, 0], T[t, 2] - T[t, 0])
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    p = p + nrm * rng.uniform(-0.03, 0.03, (n, 1))
    return p.astype(np.float32).astype(np.float64)


REGION_NAMES = ("a", "b", "ab", "c", "ac", "bc", "face")
FORCED_TRIANGLES = (0, 2 * (1 * NV + 1), 2 * (2 * NV + 2) + 1, 2 * (3 * NV + 7), 2 * (11 * NV + 5) + 1)   # materials 0, 1, 2, none, 2


def forced_points(V, F):
    """37 (point, triangle) pairs: for five triangles one point in each Voronoi region (3 vertices, 3 edges, the face), off the
    plane too, and two more face points."""
    T = V[F]
    P, idx = [], []
    for t in FORCED_TRIANGLES:
        a, b, c = T[t]
        n = np.cross(b - a, c - a)
        n /= np.linalg.norm(n)
        out = lambda s, e, o: np.cross(e - s, n) * (1 if np.dot(np.cross(e - s, n), o - s) < 0 else -1)    # noqa: E731
        P += [a + 0.3 * (a - b) + 0.3 * (a - c) + 0.02 * n, b + 0.3 * (b - a) + 0.3 * (b - c) - 0.03 * n,
              (a + b) / 2 + 0.4 * out(a, b, c) + 0.01 * n, c + 0.3 * (c - a) + 0.3 * (c - b) + 0.02 * n,
              (a + c) / 2 + 0.4 * out(a, c, b) - 0.02 * n, 0.4 * b + 0.6 * c + 0.4 * out(b, c, a) + 0.01 * n,
              0.5 * a + 0.2 * b + 0.3 * c - 0.04 * n]
        idx += [t] * 7
    for t, w in ((2 * (0 * NV + 5), (0.2, 0.7, 0.1)), (2 * (4 * NV + 3) + 1, (0.6, 0.15, 0.25))):
        P.append((T[t] * np.array(w)[:, None]).sum(0))
        idx.append(t)
    return np.array(P).astype(np.float32).astype(np.float64), np.array(idx, dtype=np.int64)


# ------------------------------------------------------------------------------------------------ the kernel, restated
def _dot(x, y):
    p = x * y
    return (p[:, 0] + p[:, 1]) + p[:, 2]


def closest_point_and_region(tri, p):
    """(hit f64 [n,3], region index into REGION_NAMES [n]) - step 1 of wisp_mesh_closest_tex."""
    a, b, c = tri[:, 0], tri[:, 1], tri[:, 2]
    ab, ac = b - a, c - a
    d1, d2 = _dot(ab, p - a), _dot(ac, p - a)
    d3, d4 = _dot(ab, p - b), _dot(ac, p - b)
    d5, d6 = _dot(ab, p - c), _dot(ac, p - c)
    va, vb, vc = d3 * d6 - d5 * d4, d5 * d2 - d1 * d6, d1 * d4 - d3 * d2
    inv = 1.0 / ((va + vb) + vc)
    cands = [a, b, a + (d1 / (d1 - d3))[:, None] * ab, c, a + (d2 / (d2 - d6))[:, None] * ac,
             b + ((d4 - d3) / ((d4 - d3) + (d5 - d6)))[:, None] * (c - b),
             (a + ab * (vb * inv)[:, None]) + ac * (vc * inv)[:, None]]
    conds = [(d1 <= 0) & (d2 <= 0), (d3 >= 0) & (d4 <= d3), (vc <= 0) & (d1 >= 0) & (d3 <= 0), (d6 >= 0) & (d5 <= d6),
             (vb <= 0) & (d2 >= 0) & (d6 <= 0), (va <= 0) & ((d4 - d3) >= 0) & ((d5 - d6) >= 0)]
    hit, region = cands[6], torch.full((p.shape[0],), 6, dtype=torch.int64)
    for k in reversed(range(6)):
        hit = torch.where(conds[k][:, None], cands[k], hit)
        region = torch.where(conds[k], torch.full_like(region, k), region)
    return hit, region


def _source_index(g, size):
    """wisp_reflect_source_index (csrc/grid_sample_dev.h) in fp32."""
    span = float(size - 1)
    if span <= 0:
        return torch.zeros_like(g)
    x = ((g + 1.0) * 0.5 * span).abs()
    flips = torch.floor(x / span)
    extra = x - flips * span
    x = torch.where(flips.to(torch.int64) % 2 == 1, span - extra, extra)
    return x.clamp(0.0, span)


def sample_tex_ref(uv, material, mats):
    """Step 4 + the zero rule of step 5: uv f32 [n,2], material i64 [n] -> rgb f32 [n,3]."""
    uv = uv.to(torch.float32)
    rgb = torch.zeros(uv.shape[0], 3, dtype=torch.float32)
    for i, mat in mats.items():
        sel = material == i
        if not bool(sel.any()):
            continue
        if 'diffuse_texname' not in mat:
            rgb[sel] = torch.as_tensor(mat.get('diffuse', [0.0, 0.0, 0.0]), dtype=torch.float32)
            continue
        tex = mat['diffuse_texname'][..., :3].to(torch.float32)
        h, w = tex.shape[:2]
        gx, gy = uv[sel, 0] * 2.0 - 1.0, -(uv[sel, 1] * 2.0 - 1.0)
        ix, iy = _source_index(gx, w), _source_index(gy, h)
        fx, fy = torch.floor(ix), torch.floor(iy)
        x0, y0 = fx.long(), fy.long()
        wx1, wx0, wy1, wy0 = ix - fx, (fx + 1.0) - ix, iy - fy, (fy + 1.0) - iy
        vx1, vy1 = (x0 + 1 < w), (y0 + 1 < h)
        x1, y1 = (x0 + 1).clamp(max=w - 1), (y0 + 1).clamp(max=h - 1)
        zero = torch.zeros(1, dtype=torch.float32)
        acc = tex[y0, x0] * (wx0 * wy0)[:, None]
        acc = acc + torch.where(vx1[:, None], tex[y0, x1] * (wx1 * wy0)[:, None], zero)
        acc = acc + torch.where(vy1[:, None], tex[y1, x0] * (wx0 * wy1)[:, None], zero)
        acc = acc + torch.where((vx1 & vy1)[:, None], tex[y1, x1] * (wx1 * wy1)[:, None], zero)
        rgb[sel] = acc
    return rgb


def closest_tex_ref(points, mesh, tidx, texv, texf, mats):
    """(hit f64 [n,3], rgb f32 [n,3], uv f32 [n,2]) of wisp_mesh_closest_tex for torch CPU inputs."""
    points, mesh = points.to(torch.float64), mesh.to(torch.float64)
    tidx = tidx.to(torch.int64)
    have = (tidx >= 0) & (tidx < mesh.shape[0])
    t = torch.where(have, tidx, torch.zeros_like(tidx))
    tri = mesh[t]
    hit, _ = closest_point_and_region(tri, points)
    a, ab, ac, r = tri[:, 0], tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0], hit - tri[:, 0]
    d00, d01, d11, d20, d21 = _dot(ab, ab), _dot(ab, ac), _dot(ac, ac), _dot(r, ab), _dot(r, ac)
    denom = d00 * d11 - d01 * d01
    l1 = ((d11 * d20 - d01 * d21) / denom).clamp(0.0, 1.0).to(torch.float32)
    l2 = ((d00 * d21 - d01 * d20) / denom).clamp(0.0, 1.0).to(torch.float32)
    l0 = (1.0 - (l1 + l2)).clamp(0.0, 1.0)
    tf = texf[t]
    material = torch.where(have, tf[:, 3], torch.full_like(t, -1))
    k = tf[:, :3]
    ok = ((k >= 0) & (k < texv.shape[0])).all(dim=1)
    tvv = texv.to(torch.float32)[k.clamp(0, max(texv.shape[0] - 1, 0))] if texv.shape[0] else torch.zeros(t.shape[0], 3, 2)
    uv = (tvv[:, 0] * l0[:, None] + tvv[:, 1] * l1[:, None]) + tvv[:, 2] * l2[:, None]
    mapped = torch.zeros_like(have)
    for i, mat in mats.items():
        if 'diffuse_texname' in mat:
            mapped |= material == i
    material = torch.where(mapped & ~ok, torch.full_like(material, -1), material)
    return hit, sample_tex_ref(uv, material, mats), uv


# ------------------------------------------------------------------------------------------------ the reference, in place
def have_reference():
    return os.path.isfile(os.path.join(REF, "wisp/ops/mesh/closest_tex.py"))


def _exec_reference(rel, inject=None):
    path = os.path.join(REF, rel)
    src = open(path).read()
    src = re.sub(r"^import wisp\._C as _C\s*$", "", src, flags=re.M)
    src = re.sub(r"^from \.\w+ import \w+\s*$", "", src, flags=re.M)           # siblings are injected below
    ns = {"__name__": "reference_" + os.path.basename(path)}
    ns.update(inject or {})
    exec(compile(src, path, "exec"), ns)
    return ns


def reference_closest_tex(V32, F, texv, texf, mats, points32, forced_tidx=None):
    """The reference's closest_tex (closest_tex.py, with its own closest_point.py, barycentric_coordinates.py and sample_tex.py)
    executed where it lies on torch CPU tensors.  The CUDA extension behind closest_point is replaced by tests/mesh_sdf_oracle.py
    (nearest triangle and signed distance), `forced_tidx` [k] overrides the triangle of the LAST k points, and Tensor.cuda() is a
    no-op for the duration.  -> (rgb f32 [n,3], hit f64 [n,3], dist f64 [n], tidx i64 [n])."""
    mesh = V32.double()[F].numpy()
    seen = {}

    def mesh_to_sdf_triangle_cuda(p, m):
        sdf, idx, _, _ = oracle.mesh_sdf(p.numpy(), mesh)
        if forced_tidx is not None and len(forced_tidx):
            idx[-len(forced_tidx):] = np.asarray(forced_tidx)
        seen['tidx'] = torch.from_numpy(idx.copy())
        return [torch.from_numpy(np.concatenate([sdf, idx.astype(np.float64)]))]

    stub = types.SimpleNamespace(external=types.SimpleNamespace(mesh_to_sdf_triangle_cuda=mesh_to_sdf_triangle_cuda))
    saved = torch.Tensor.cuda
    torch.Tensor.cuda = lambda self, *a, **k: self
    try:
        cp = _exec_reference("wisp/ops/mesh/closest_point.py", {"_C": stub})
        bary = _exec_reference("wisp/ops/mesh/barycentric_coordinates.py")["barycentric_coordinates"]
        samp = _exec_reference("wisp/ops/mesh/sample_tex.py")["sample_tex"]
        fn = _exec_reference("wisp/ops/mesh/closest_tex.py", {"closest_point": cp["closest_point"], "barycentric_coordinates": bary,
                                                              "sample_tex": samp})["closest_tex"]
        rgb, hit, dist = fn(V32, F, texv, texf, mats, points32)
    finally:
        torch.Tensor.cuda = saved
    return rgb, hit, dist, seen['tidx']


def load_golden():
    return {k: v for k, v in np.load(GOLDEN).items()}


def mats_from_golden(g):
    return {0: {'diffuse': torch.from_numpy(g['kd0']), 'diffuse_texname': torch.from_numpy(g['map0'])},
            1: {'diffuse': torch.from_numpy(g['kd1'])},
            2: {'diffuse': torch.from_numpy(g['kd2']), 'diffuse_texname': torch.from_numpy(g['map2'])}}
