"""CPU: SPC rendering without a GPU.
  * the reference's own SPCField / PackedSPCTracer / wisp.ops.pointcloud bodies, executed where they lie over the oracle's
    restatement of the Kaolin leaves, against tests/spc_render_ref.py and against this package's classes (skipped where the
    reference tree is not mounted);
  * wisp_spc_first_hit: declared, bound, exported; every argument check answers before a launch; the kernel's resources;
  * the inputs of tests/test_gpu_spc_first_hit.py really reach the walk's hard paths (back-ups, exhausted trees);
  * the barycentric mesh sampler."""
import ctypes
import os
import re
import sys
import types

import numpy as np
import pytest
import torch

import gpu_helpers as gh
import kernel_meta
import spc_render_ref as ref
from oracle import spc as ospc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "kaolin-wisp_amd", "csrc", "libwisp_hip.so")
REF = "/root/reference/wisp"
needs_reference = pytest.mark.skipif(not os.path.isdir(REF), reason="reference tree not mounted")
t = torch.from_numpy


# ------------------------------------------------------------------------------------------------ reference in place
def _exec_reference(rel):
    """module namespace of a reference source file executed where it lies (as tests/test_reference_modules.py does)"""
    path = os.path.join(REF, rel)
    name = "reference_" + rel.replace("/", "_").replace(".py", "")
    mod = types.ModuleType(name)
    mod.__file__ = path
    sys.modules[name] = mod
    exec(compile(open(path).read(), path, "exec"), mod.__dict__)
    return mod.__dict__


def _oracle_raytrace(self, rays, level=None, with_exit=False, begun=None):
    """OctreeAS.raytrace on the host: the oracle's traversal (what kaolin's unbatched_raytrace is restated as)."""
    from wisp.accelstructs import ASRaytraceResults
    level = self.max_level if level is None else level
    ridx, pidx, depth = ospc.raytrace(self.octree.numpy(), self.points.numpy(), self.pyramid.numpy(), self.prefix.numpy(),
                                      rays.origins.numpy(), rays.dirs.numpy(), level, with_exit=with_exit)
    return ASRaytraceResults(ridx=t(ridx), pidx=t(pidx), depth=t(depth.copy()))


@pytest.fixture
def reference_spc(monkeypatch):
    """(reference SPCField, reference PackedSPCTracer): the Kaolin leaves are the oracle's, OctreeAS.raytrace is the oracle's."""
    from wisp.accelstructs import OctreeAS
    import wisp.ops.render as render_ops

    def scan_octrees(octree, lengths):
        lvl, pyramid, exsum = ospc.scan_octree(octree.numpy())
        return lvl, t(np.asarray(pyramid))[None], t(np.asarray(exsum))
    k = types.ModuleType("kaolin")
    k.ops = types.ModuleType("kaolin.ops")
    k.ops.spc = types.ModuleType("kaolin.ops.spc")
    k.ops.spc.scan_octrees = scan_octrees
    k.ops.spc.generate_points = lambda octree, pyramid, exsum: t(ospc.generate_points(octree.numpy(), pyramid[0].numpy(), exsum.numpy()))
    k.ops.spc.unbatched_get_level_points = lambda points, pyramid, level: points[int(pyramid[1, level]):int(pyramid[1, level]) + int(pyramid[0, level])]
    k.render = types.ModuleType("kaolin.render")
    k.render.spc = types.ModuleType("kaolin.render.spc")
    k.render.spc.mark_pack_boundaries = lambda ridx: t(ospc.mark_pack_boundaries(ridx.numpy()))
    k._C = types.ModuleType("kaolin._C")
    for name, mod in {"kaolin": k, "kaolin.ops": k.ops, "kaolin.ops.spc": k.ops.spc, "kaolin.render": k.render,
                      "kaolin.render.spc": k.render.spc, "kaolin._C": k._C}.items():
        monkeypatch.setitem(sys.modules, name, mod)
    monkeypatch.setattr(OctreeAS, "raytrace", _oracle_raytrace)
    monkeypatch.setattr(render_ops, "mark_pack_boundaries", lambda ridx: t(ospc.mark_pack_boundaries(ridx.numpy())))
    return _exec_reference("models/nefs/spc_field.py")["SPCField"], _exec_reference("tracers/packed_spc_tracer.py")["PackedSPCTracer"]


def _scene(seed=3, level=4, n=260):
    rng = np.random.default_rng(seed)
    octree = ospc.points_to_octree(rng.integers(0, 2 ** level, size=(n, 3)), level)
    points, pyramid, exsum = ospc.octree_to_spc(octree)
    cells = int(pyramid[0, level])
    colors = rng.integers(0, 256, size=cells * 4).astype(np.uint8)
    normals = rng.normal(size=(cells, 3)).astype(np.float32)
    normals /= np.linalg.norm(normals, axis=1, keepdims=True)
    return octree, pyramid, colors, normals


def _features(source, colors, normals):
    return {"colors": dict(colors=t(colors)), "normals": dict(normals=t(normals)), "coords": None,
            "both": dict(colors=t(colors), normals=t(normals))}[source]


def _same_buffers(rb, want, what):
    assert rb.depth.dtype == torch.float32 and tuple(rb.depth.shape) == want["depth"].shape, what
    assert rb.hit.dtype == torch.bool and tuple(rb.hit.shape) == want["hit"].shape, what
    assert tuple(rb.rgb.shape) == want["rgb"].shape and tuple(rb.alpha.shape) == want["alpha"].shape, what
    assert np.array_equal(rb.depth.numpy().view(np.uint32), want["depth"].view(np.uint32)), what
    assert np.array_equal(rb.hit.numpy(), want["hit"]), what
    assert np.array_equal(rb.rgb.numpy().view(np.uint32), want["rgb"].view(np.uint32)), what
    assert np.array_equal(rb.alpha.numpy().view(np.uint32), want["alpha"].view(np.uint32)), what


@needs_reference
@pytest.mark.parametrize("source", ["colors", "normals", "coords", "both"])
def test_reference_field_and_tracer_bodies_equal_the_restatement_and_the_package_classes(reference_spc, source):
    """SPCField.__init__ / init_grid / rgba and PackedSPCTracer.trace from the reference files, the package's classes (modular
    path, on the host over the same stand-ins) and spc_render_ref: colours, rgba and all four buffers bit for bit - on a batch
    with hits and misses, a batch where every ray misses and an empty batch."""
    from wisp.core import Rays
    from wisp.models.nefs import SPCField
    from wisp.tracers import PackedSPCTracer
    RefField, RefTracer = reference_spc
    octree, pyramid, colors, normals = _scene()
    level = pyramid.shape[1] - 2
    want_colors = ref.field_colors(octree, colors if source in ("colors", "both") else None,
                                   normals if source in ("normals", "both") else None)
    fields = dict(reference=RefField(t(octree), _features(source, colors, normals), device='cpu'),
                  package=SPCField(t(octree), _features(source, colors, normals), device='cpu'))
    for who, nef in fields.items():
        assert nef.colors.dtype == torch.float32 and np.array_equal(nef.colors.numpy().view(np.uint32), want_colors.view(np.uint32)), who
        assert nef.get_supported_channels() == {"rgb"} and str(nef.device) == 'cpu' and set(nef.public_properties()) == {"Grid"}, who
        assert nef.grid.num_lods == 0 and nef.grid.feature_dim == 3 and nef.grid.blas.max_level == level, who
        pick = np.random.default_rng(5).integers(int(pyramid[1, level]), int(pyramid[1, level + 1]), size=37)
        got = nef(ridx_hit=t(pick), channels="rgb")
        assert tuple(got.shape) == (37, 1, 3) and np.array_equal(got.numpy(), ref.rgba(want_colors, pyramid, pick)), who

    o, d = gh.make_rays(300, 11)
    away = (o * 1.5).astype(np.float32), o.copy()                         # pointing away from the cube: no ray hits it
    batches = dict(mixed=(o, d), all_miss=away, empty=(np.zeros((0, 3), np.float32), np.zeros((0, 3), np.float32)))
    tracers = dict(reference=RefTracer(), package=PackedSPCTracer())
    assert tracers["package"].get_supported_channels() == tracers["reference"].get_supported_channels() == {"depth", "hit", "rgb", "alpha"}
    assert tracers["package"].get_required_nef_channels() == tracers["reference"].get_required_nef_channels() == {"rgb"}
    for name, (bo, bd) in batches.items():
        want = ref.trace(octree, want_colors, bo, bd)
        if name == "mixed":
            assert 0 < want["hit"].sum() < want["hit"].shape[0]
        if name == "all_miss":
            assert not want["hit"].any()
        for who in ("reference", "package"):
            rb = tracers[who](fields[who], rays=Rays(t(bo), t(bd), dist_min=0.0, dist_max=6.0), channels=["rgb", "depth"])
            _same_buffers(rb, want, (source, name, who))


@needs_reference
def test_pointcloud_ops_equal_the_reference_function_bodies():
    from wisp.core import Rays
    import wisp.ops.pointcloud as mine
    ref_norm = _exec_reference("ops/pointcloud/processing.py")["normalize_pointcloud"]
    ref_conv = _exec_reference("ops/pointcloud/conversions.py")["create_pointcloud_from_images"]
    rng = np.random.default_rng(8)
    cloud = t((rng.normal(size=(500, 3)) * [1.0, 3.0, 0.5] + [4.0, -2.0, 1.0]).astype(np.float32))
    want = ref_norm(cloud.clone(), return_scale=True)
    got = mine.normalize_pointcloud(cloud.clone(), return_scale=True)
    for a, b in zip(got, want):
        assert torch.equal(torch.as_tensor(a), torch.as_tensor(b))
    assert torch.equal(mine.normalize_pointcloud(cloud.clone()), ref_norm(cloud.clone()))
    # the scale is 1 / (largest centred COORDINATE): the longest axis ends exactly at +1, nothing leaves [-1, 1]
    assert float(got[0].max()) == 1.0 and float(got[0].abs().max()) <= 1.0 + 1e-6
    views = 3
    rgbs = [t(rng.uniform(size=(6, 5, 4)).astype(np.float32)) for _ in range(views)]
    masks = [t((rng.uniform(size=(6, 5, 1)) > 0.4).astype(np.float32)) for _ in range(views)]
    masks[1] = torch.zeros(6, 5, 1)                                       # a view without a single valid pixel
    depths = [t(rng.uniform(1, 3, size=(6, 5, 1)).astype(np.float32)) for _ in range(views)]
    rays = [Rays(t(rng.normal(size=(6, 5, 3)).astype(np.float32)), t(rng.normal(size=(6, 5, 3)).astype(np.float32))) for _ in range(views)]
    wc, wk = ref_conv(rgbs, masks, rays, depths)
    gc, gk = mine.create_pointcloud_from_images(rgbs, masks, rays, depths)
    assert torch.equal(gc, wc) and torch.equal(gk, wk)
    assert gc.shape == (int(sum(m.sum() for m in masks)), 3) and gk.shape == gc.shape


# ------------------------------------------------------------------------------------------------ entry point and kernel
def test_first_hit_entry_point_is_declared_bound_and_exported_alike():
    import wisp._C as C
    header = open(os.path.join(ROOT, "include", "wisp_hip.h")).read()
    header = re.sub(r"/\*.*?\*/", " ", header, flags=re.S)
    m = re.search(r"\bint\s+wisp_spc_first_hit\s*\(([^)]*)\)\s*;", header)
    assert m, "wisp_spc_first_hit is not declared in include/wisp_hip.h"
    args = [" ".join(a.split()) for a in m.group(1).split(",")]
    names = [a.rsplit(" ", 1)[1].lstrip("*") for a in args]
    assert names == ["octree", "points", "exsum", "origins", "dirs", "num_rays", "level", "colors", "color_stride", "level_first",
                     "pidx", "depth", "rgb", "alpha", "hit", "stream"]
    kinds = ["ptr" if ("*" in a or a.startswith("wisp_stream_t")) else {"int64_t": "i64", "int": "i32", "int32_t": "i32"}[a.rsplit(" ", 1)[0]]
             for a in args]
    bound = [{ctypes.c_void_p: "ptr", ctypes.c_int64: "i64", ctypes.c_int32: "i32"}[c] for c in C.SIGNATURES["wisp_spc_first_hit"]]
    assert kinds == bound
    assert hasattr(ctypes.CDLL(LIB), "wisp_spc_first_hit")
    assert C.lib.wisp_abi_version() == 4 == C.ABI_VERSION                 # an added entry point does not bump the version


def test_first_hit_argument_checks_answer_before_any_launch():
    """Every refusal comes back as an error code with a message, on a machine without a GPU: nothing was launched."""
    import wisp._C as C
    fn = C.lib.wisp_spc_first_hit
    P = ctypes.c_void_p
    buf = (ctypes.c_uint8 * 256)()
    p = P(ctypes.addressof(buf))                                          # a non-null address; never dereferenced by a refused call
    null = P(0)

    def call(octree=p, points=p, exsum=p, origins=p, dirs=p, R=4, level=3, colors=null, stride=0, first=0, pidx=p, depth=p,
             rgb=null, alpha=null, hit=null):
        return fn(octree, points, exsum, origins, dirs, R, level, colors, stride, first, pidx, depth, rgb, alpha, hit, null)

    for kw, msg in ((dict(octree=null), "null pointer"), (dict(points=null), "null pointer"), (dict(exsum=null), "null pointer"),
                    (dict(origins=null), "null pointer"), (dict(dirs=null), "null pointer"), (dict(pidx=null), "null pointer"),
                    (dict(depth=null), "null pointer"), (dict(level=-1), "level"), (dict(level=16), "level"), (dict(R=-1), "num_rays"),
                    (dict(R=2 ** 31), "num_rays"), (dict(colors=p, stride=2, rgb=p), "color_stride"),
                    (dict(colors=p, stride=0, rgb=p), "color_stride"), (dict(colors=p, stride=4), "without an rgb"),
                    (dict(rgb=p), "needs colors"), (dict(first=-1), "level_first")):
        assert call(**kw) != 0, kw
        assert msg in C.last_error(), (kw, C.last_error())
    assert call(R=0) == 0                                                 # an empty batch is not an error and launches nothing
    assert call(R=0, octree=null, points=null, pidx=null, depth=null) == 0


def test_first_hit_binding_refuses_cpu_tensors_and_narrow_colors():
    import wisp._C as C
    from wisp.accelstructs import OctreeAS
    from wisp.core import Rays
    blas = OctreeAS.make_dense(2)
    with pytest.raises(RuntimeError, match="GPU tensor"):
        blas.first_hit(Rays(torch.zeros(4, 3), torch.ones(4, 3)))
    assert "first_hit" in OctreeAS.__dict__ and "raytrace" in OctreeAS.__dict__


@pytest.mark.skipif(not kernel_meta.available(LIB), reason="library or llvm-readelf missing")
def test_first_hit_kernel_resources():
    """No scratch; LDS = the pending-sibling stack, two 32-bit words (base, packed state) per level 0..14 and ray, 32 rays per
    workgroup; 8 lanes per ray -> a workgroup of 256."""
    meta = {n: v for n, v in kernel_meta.kernels(LIB).items() if "spc_first_hit_kernel" in n}
    assert len(meta) == 1, sorted(meta)
    (k,) = meta.values()
    rays_per_group, stack_levels = 32, 15
    assert k["scratch"] == 0
    assert k["lds"] == 2 * 4 * stack_levels * rays_per_group == 3840
    assert k["wg"] == 8 * rays_per_group == 256


# ------------------------------------------------------------------------------------------------ the GPU tests' inputs
@pytest.mark.parametrize("tree,min_backtrack_share", [((5, 2500, 31), 0.5), ((7, 40000, 32), 0.5)])
def test_gpu_inputs_make_the_walk_back_up(tree, min_backtrack_share):
    octree, points, pyramid, exsum = gh.sparse_tree(*tree)
    o, d = gh.make_rays(700, 33)
    s = ref.traversal_stats(octree, points, pyramid, exsum, o, d, tree[0])
    print(tree, s)
    assert s["hitting"] >= 600 and s["backtrack"] >= min_backtrack_share * s["hitting"], s


def test_gpu_inputs_make_rays_exhaust_the_tree():
    octree, points, pyramid, exsum = gh.sparse_tree(3, 40, 5)
    o, d = gh.make_rays(700, 33)
    s = ref.traversal_stats(octree, points, pyramid, exsum, o, d, 3)
    print(s)
    assert s["enter_and_miss"] >= 700 // 4 and s["hitting"] >= 100 and s["backtrack"] >= 1, s


# ------------------------------------------------------------------------------------------------ mesh sampler
def test_barycentric_surface_samples_lie_on_their_face_and_carry_their_weights():
    from wisp.ops import mesh as mesh_ops
    torch.manual_seed(4)
    rng = np.random.default_rng(4)
    V = t(rng.normal(size=(12, 3)))                                       # float64: the on-the-face residuals are rounding only
    F = t(rng.integers(0, 12, size=(9, 3)))
    F = F[(F[:, 0] != F[:, 1]) & (F[:, 1] != F[:, 2]) & (F[:, 0] != F[:, 2])]
    uv = t(rng.uniform(size=(F.shape[0], 3, 2)))
    pts, fidx, w = mesh_ops.sample_surface_barycentric(V, F, 4000)
    assert pts.shape == (4000, 3) and fidx.shape == (4000,) and w.shape == (4000, 3) and fidx.dtype == torch.int64
    assert int(fidx.min()) >= 0 and int(fidx.max()) < F.shape[0]
    assert float(w.min()) >= 0.0 and float((w.sum(1) - 1).abs().max()) <= 1e-6
    tri = V[F[fidx]]
    assert float((pts - (w[:, :, None] * tri).sum(1)).abs().max()) <= 1e-12
    n = torch.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0], dim=1)
    n = n / n.norm(dim=1, keepdim=True)
    assert float(((pts - tri[:, 0]) * n).sum(1).abs().max()) <= 1e-9      # in the triangle's plane (inside it: convex weights)
    got_uv = (w[:, :, None].to(uv.dtype) * uv[fidx]).sum(1)               # what mesh2spc does with the texture coordinates
    lo, hi = uv[fidx].min(1)[0], uv[fidx].max(1)[0]
    assert bool(((got_uv >= lo - 1e-6) & (got_uv <= hi + 1e-6)).all())
    corner = w.argmax(1)                                                  # a sample near a corner has that corner's uv
    near = w.max(1)[0] > 0.98
    assert bool(near.any())
    assert float((got_uv[near] - uv[fidx[near], corner[near]]).abs().max()) <= 0.05


def test_barycentric_surface_samples_are_area_weighted():
    """Two triangles of areas 3 : 1, 20000 draws: the larger one's share is binomial(20000, 0.75), sigma = sqrt(0.75 * 0.25 /
    20000) = 0.00306; the bar is 5 sigma = 0.0153."""
    from wisp.ops import mesh as mesh_ops
    torch.manual_seed(7)
    V = torch.tensor([[0.0, 0, 0], [3.0, 0, 0], [0.0, 2, 0], [0.0, 0, 1], [1.0, 0, 1], [0.0, 2, 1]])
    F = torch.tensor([[0, 1, 2], [3, 4, 5]])
    _, fidx, _ = mesh_ops.sample_surface_barycentric(V, F, 20000)
    share = float((fidx == 0).float().mean())
    print("share of the larger triangle", share)
    assert abs(share - 0.75) <= 5 * (0.75 * 0.25 / 20000) ** 0.5
