"""GPU: wisp_spc_first_hit, OctreeAS.first_hit, SPCField, PackedSPCTracer and the SPC scripts.

The kernel is pinned bit for bit by the CPU oracle (the first nugget per ray of oracle.spc.raytrace) and by the package's own
raytrace; tests/test_spc_render_host.py shows on the CPU that the trees and rays used here make the walk back up (555 of 685 and
636 of 688 hitting rays) and exhaust the tree (246 of 700 rays enter a root child and hit no leaf)."""
import functools
import json
import os
import sys

import numpy as np
import pytest
import torch

import spc_render_ref as ref
from gpu_helpers import DEV, _C, cuda, make_rays, sparse_tree
from oracle import spc as ospc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bits(x):
    x = x.detach().cpu().numpy() if torch.is_tensor(x) else np.asarray(x)
    return x.view(np.uint32) if x.dtype == np.float32 else x


# ------------------------------------------------------------------------------------------------ shared inputs, computed once
@functools.lru_cache(maxsize=None)
def _tree(name):
    if name == "level0":
        oc = np.zeros(0, dtype=np.uint8)
    elif name == "level1_one_child":
        oc = ospc.points_to_octree(np.array([[1, 0, 1]]), 1)
    elif name == "dense3":
        oc = ospc.create_dense_octree(3)
    else:
        return sparse_tree(*{"sparse5": (5, 2500, 31), "sparse7": (7, 40000, 32), "sparse3": (3, 40, 5)}[name])
    return (oc,) + ospc.octree_to_spc(oc)


TREES = ("level0", "level1_one_child", "dense3", "sparse5", "sparse7", "sparse3")


@functools.lru_cache(maxsize=None)
def _case(name):
    """(tree, level, origins, dirs, oracle first hit) with 700 rays: [0:3] axis aligned (infinite inverses), [3] origin inside
    the volume, [4] origin at the centre of an occupied leaf (entry depth 0), [5:9] rays that miss the cube."""
    oc, pts, pyr, ex = _tree(name)
    level = pyr.shape[1] - 2
    o, d = make_rays(700, 33)
    d[:3] = [[1, 0, 0], [0, -1, 0], [0, 0, 1]]
    o[:3] = [[-3, 0.13, 0.27], [0.4, 3, -0.2], [0.05, 0.05, -3]]
    o[3] = [0.01, 0.02, 0.03]
    leaf = pts[int(pyr[1, level]) + int(pyr[0, level]) // 2].astype(np.float32)
    o[4] = (2.0 * leaf + 1.0) / np.float32(2 ** level) - 1.0
    o[5:9] = 5.0
    d[5:9] = [1, 0, 0]
    want = ref.first_hit(oc, pts, pyr, ex, o, d, level)
    for a in (o, d) + want:
        a.setflags(write=False)
    return (oc, pts, pyr, ex), level, o, d, want


def _run(tree, level, o, d, **kw):
    oc, pts, pyr, ex = tree
    return _C().spc_first_hit(cuda(oc), cuda(pts), cuda(ex), cuda(o), cuda(d), level, **kw)


# ------------------------------------------------------------------------------------------------ 1. against the oracle
@pytest.mark.parametrize("rays", [1, 31, 33, 700])
@pytest.mark.parametrize("name", TREES)
def test_first_hit_equals_the_oracles_first_nugget_bit_for_bit(name, rays):
    tree, level, o, d, (want_pidx, want_depth, want_hit) = _case(name)
    pidx, depth, rgb, alpha, hit = _run(tree, level, o[:rays], d[:rays], want_hit=True)
    assert rgb is None and alpha is None
    assert pidx.dtype == torch.int32 and pidx.shape == (rays,) and depth.dtype == torch.float32 and depth.shape == (rays, 1)
    assert hit.dtype == torch.bool and hit.shape == (rays,)
    assert np.array_equal(pidx.cpu().numpy(), want_pidx[:rays])
    assert np.array_equal(_bits(depth), _bits(want_depth[:rays]))
    assert np.array_equal(hit.cpu().numpy(), want_hit[:rays])
    if rays == 700:
        assert not want_hit[5:9].any()                                    # the four rays beside the cube
        assert want_hit[4] and want_depth[4, 0] == 0.0                    # the origin inside an occupied leaf enters at depth 0
        assert want_hit.sum() >= (50 if name != "level1_one_child" else 1)


# ------------------------------------------------------------------------------------------------ 2. against the package's raytrace
@functools.lru_cache(maxsize=None)
def _torus_blas(level=8, n=400000, seed=2):
    from wisp.accelstructs import OctreeAS
    rng = np.random.default_rng(seed)
    a, b = rng.uniform(0, 2 * np.pi, n), rng.uniform(0, 2 * np.pi, n)
    cloud = np.stack([(0.6 + 0.25 * np.cos(b)) * np.cos(a), (0.6 + 0.25 * np.cos(b)) * np.sin(a), 0.25 * np.sin(b)], 1).astype(np.float32)
    return OctreeAS.from_pointcloud(cuda(cloud), level)


def _look_at_rays(h, w):
    from wisp.ops.raygen import LookAtCamera, generate_centered_pixel_coords, generate_pinhole_rays
    cam = LookAtCamera(eye=(1.1, -1.4, 1.2), at=(0.0, 0.0, 0.0), up=(0.0, 0.0, 1.0), fov=float(np.radians(45.0)), width=w, height=h,
                       device=DEV)
    return generate_pinhole_rays(cam, generate_centered_pixel_coords(w, h, device=DEV))


def test_first_hit_equals_the_first_nugget_of_the_packages_raytrace_on_a_level_8_torus():
    from wisp.ops.render import mark_pack_boundaries
    blas = _torus_blas()
    rays = _look_at_rays(64, 64)
    rt = blas.raytrace(rays, 8)
    first = mark_pack_boundaries(rt.ridx)
    want_pidx = torch.full((4096,), -1, dtype=torch.int32, device=DEV)
    want_depth = torch.zeros(4096, 1, device=DEV)
    want_pidx[rt.ridx[first].long()] = rt.pidx[first]
    want_depth[rt.ridx[first].long()] = rt.depth[first]
    pidx, depth = blas.first_hit(rays)                                    # level=None: the finest
    assert torch.equal(pidx, want_pidx) and np.array_equal(_bits(depth), _bits(want_depth))
    hitting = int((want_pidx >= 0).sum())
    assert 400 <= hitting < 4096 and rt.ridx.shape[0] >= 2 * hitting       # a shell: several nuggets behind every first one
    lo = int(blas.pyramid[1, 8])
    assert int(pidx[pidx >= 0].min()) >= lo and int(pidx.max()) < lo + int(blas.pyramid[0, 8])
    coarse = blas.first_hit(rays, level=5)[0]                             # another level through the public method
    rt5 = blas.raytrace(rays, 5)
    f5 = mark_pack_boundaries(rt5.ridx)
    want5 = torch.full((4096,), -1, dtype=torch.int32, device=DEV)
    want5[rt5.ridx[f5].long()] = rt5.pidx[f5]
    assert torch.equal(coarse, want5)


# ------------------------------------------------------------------------------------------------ 3. output buffers
GUARD = 64


def _guarded(rows, cols, dtype, fill):
    """(whole buffer, interior view): `rows` x `cols` of `dtype` between two guard regions of GUARD elements, all set to `fill`"""
    whole = torch.full((rows * cols + 2 * GUARD,), fill, dtype=dtype, device=DEV)
    return whole, whole[GUARD:GUARD + rows * cols]


def _raw_call(tree, level, o, d, colors, stride, level_first, with_rgb, with_alpha, with_hit):
    C = _C()
    oc, pts, pyr, ex = (cuda(a) for a in tree)
    O, D = cuda(o), cuda(d)
    R = o.shape[0]
    bufs = dict(pidx=_guarded(R, 1, torch.int32, -7), depth=_guarded(R, 1, torch.float32, float("nan")))
    if with_rgb:
        bufs["rgb"] = _guarded(R, 3, torch.float32, float("nan"))
    if with_alpha:
        bufs["alpha"] = _guarded(R, 1, torch.float32, float("nan"))
    if with_hit:
        bufs["hit"] = _guarded(R, 1, torch.uint8, 0xFF)
    p = lambda k: C._p(bufs[k][1]) if k in bufs else C._p(None)          # noqa: E731
    rc = C.lib.wisp_spc_first_hit(C._p(oc), C._p(pts), C._p(ex), C._p(O), C._p(D), R, level, C._p(colors if with_rgb else None),
                                  stride if with_rgb else 0, level_first, p("pidx"), p("depth"), p("rgb"), p("alpha"), p("hit"),
                                  C._stream())
    assert rc == 0, C.last_error()
    torch.cuda.synchronize()
    return bufs


def test_every_requested_row_is_written_and_nothing_else():
    tree, level, o, d, (want_pidx, want_depth, want_hit) = _case("sparse3")         # 246 rays walk in and find nothing
    o, d = o[:333], d[:333]                                               # a last workgroup with 13 of its 32 rays
    pyr = tree[2]
    cells, first = int(pyr[0, level]), int(pyr[1, level])
    colors = cuda(np.random.default_rng(1).uniform(0.1, 1.0, size=(cells, 4)).astype(np.float32))
    full = None
    for with_rgb, with_alpha, with_hit in ((1, 1, 1), (0, 1, 1), (1, 0, 1), (1, 1, 0), (0, 0, 0)):
        bufs = _raw_call(tree, level, o, d, colors, 4, first, with_rgb, with_alpha, with_hit)
        for k, (whole, inner) in bufs.items():
            head, tail = whole[:GUARD], whole[GUARD + inner.numel():]
            if whole.dtype == torch.float32:
                assert bool(torch.isnan(head).all()) and bool(torch.isnan(tail).all()), k          # no guard element changed
                assert not bool(torch.isnan(inner).any()), k                                         # every row overwritten
            elif whole.dtype == torch.int32:
                assert bool((head == -7).all()) and bool((tail == -7).all()) and not bool((inner == -7).any()), k
            else:
                assert bool((head == 0xFF).all()) and bool((tail == 0xFF).all()) and bool((inner <= 1).all()), k
        assert np.array_equal(bufs["pidx"][1].cpu().numpy(), want_pidx[:333])
        assert np.array_equal(_bits(bufs["depth"][1]), _bits(want_depth[:333, 0]))
        if full is None:
            full = bufs
            assert np.array_equal(bufs["hit"][1].cpu().numpy().astype(bool), want_hit[:333])
        for k in bufs:                                                    # dropping an optional output leaves the others alone
            assert torch.equal(bufs[k][1].view(torch.int32) if bufs[k][1].dtype == torch.float32 else bufs[k][1],
                               full[k][1].view(torch.int32) if full[k][1].dtype == torch.float32 else full[k][1]), k


# ------------------------------------------------------------------------------------------------ 4. colours
@pytest.mark.parametrize("stride", [3, 4])
@pytest.mark.parametrize("name", ["sparse5", "level0", "sparse3"])
def test_rgb_is_the_colour_row_of_the_first_cell(name, stride):
    tree, level, o, d, (want_pidx, _, want_hit) = _case(name)
    pyr = tree[2]
    cells, first = int(pyr[0, level]), int(pyr[1, level])
    table = np.random.default_rng(stride).normal(size=(cells, stride)).astype(np.float32)      # any bit pattern is copied as it is
    pidx, depth, rgb, alpha, hit = _run(tree, level, o, d, colors=cuda(table), level_first=first, want_alpha=True, want_hit=True)
    assert rgb.shape == (700, 3) and alpha.shape == (700, 1)
    want_rgb = np.zeros((700, 3), dtype=np.float32)
    want_rgb[want_hit] = table[want_pidx[want_hit] - first, :3]
    assert np.array_equal(pidx.cpu().numpy(), want_pidx)
    assert np.array_equal(_bits(rgb), _bits(want_rgb))
    assert np.array_equal(_bits(rgb)[~want_hit], np.zeros(((~want_hit).sum(), 3), np.uint32))   # +0.0 on misses
    assert np.array_equal(alpha.cpu().numpy()[:, 0], want_hit.astype(np.float32))
    assert np.array_equal(hit.cpu().numpy(), want_hit)


# ------------------------------------------------------------------------------------------------ 5. SPCField on the device
def _field_inputs(name="sparse5"):
    tree, level, o, d, _ = _case(name)
    cells = int(tree[2][0, level])
    rng = np.random.default_rng(17)
    colors = rng.integers(0, 256, size=cells * 4).astype(np.uint8)
    normals = rng.normal(size=(cells, 3)).astype(np.float32)
    return tree, level, o, d, colors, normals


@pytest.mark.parametrize("source", ["colors", "normals", "coords"])
def test_spc_field_colour_sources_on_the_device(source):
    from wisp.models.nefs import SPCField
    tree, level, _, _, colors, normals = _field_inputs()
    feats = {"colors": dict(colors=cuda(colors)), "normals": dict(normals=cuda(normals)), "coords": None}[source]
    nef = SPCField(cuda(tree[0]), feats, device=DEV)
    want = ref.field_colors(tree[0], colors if source == "colors" else None, normals if source == "normals" else None)
    assert nef.colors.is_cuda and nef.colors.dtype == torch.float32 and nef.device == DEV
    assert np.array_equal(_bits(nef.colors), _bits(want))
    pyr = tree[2]
    pick = np.random.default_rng(3).integers(int(pyr[1, level]), int(pyr[1, level + 1]), size=501)
    got = nef(ridx_hit=cuda(pick), channels="rgb")
    assert got.shape == (501, 1, 3) and np.array_equal(_bits(got), _bits(ref.rgba(want, pyr, pick)))


# ------------------------------------------------------------------------------------------------ 6. the tracer's two paths
@pytest.mark.parametrize("source", ["colors", "normals", "coords"])
def test_tracer_fused_and_modular_paths_agree_bit_for_bit(source, monkeypatch):
    from wisp.core import Rays
    from wisp.models import Pipeline
    from wisp.models.nefs import SPCField
    from wisp.tracers import PackedSPCTracer
    C = _C()
    tree, level, o, d, colors, normals = _field_inputs()
    feats = {"colors": dict(colors=cuda(colors)), "normals": dict(normals=cuda(normals)), "coords": None}[source]
    nef = SPCField(cuda(tree[0]), feats, device=DEV)
    want = ref.trace(tree[0], ref.field_colors(tree[0], colors if source == "colors" else None,
                                               normals if source == "normals" else None), o, d)
    rays = Rays(cuda(o), cuda(d), dist_min=0.0, dist_max=6.0)
    calls = []
    inner = C.spc_first_hit
    monkeypatch.setattr(C, "spc_first_hit", lambda *a, **k: (calls.append(1), inner(*a, **k))[1])
    pipe = Pipeline(nef, PackedSPCTracer())
    assert isinstance(pipe.tracer.fused, bool) and "fused" in vars(pipe.tracer)
    out = {}
    for fused in (True, False, True):
        pipe.tracer.fused = fused
        before = len(calls)
        rb = pipe(rays=rays, channels=["rgb", "depth", "hit", "alpha"])
        assert (len(calls) - before) == (1 if fused else 0)               # the path that ran is the path that was asked for
        assert rb.depth.shape == (700, 1) and rb.rgb.shape == (700, 3) and rb.alpha.shape == (700, 1) and rb.hit.dtype == torch.bool
        for k in ("depth", "rgb", "alpha"):
            assert np.array_equal(_bits(getattr(rb, k)), _bits(want[k])), (fused, k)
        assert np.array_equal(rb.hit.cpu().numpy(), want["hit"]), fused
        if fused in out:                                                  # a rerun is bitwise the same
            for k in ("depth", "rgb", "alpha", "hit"):
                assert torch.equal(getattr(rb, k), getattr(out[fused], k)), k
        out[fused] = rb
    # a coarser level, colours that are not plain f32 rows, and colours under optimisation take the modular path
    pipe.tracer.fused = True
    before = len(calls)
    rb = pipe(rays=rays, channels=["hit"], lod_idx=level - 1)
    oc, pts, pyr, ex = tree
    assert len(calls) == before and np.array_equal(rb.hit.cpu().numpy(), ref.first_hit(oc, pts, pyr, ex, o, d, level - 1)[2])
    kept = nef.colors
    nef.colors = kept.t().contiguous().t()                                # the same values, not contiguous
    assert not nef.colors.is_contiguous()
    rb = pipe(rays=rays, channels=["rgb"])
    assert len(calls) == before and np.array_equal(rb.hit.cpu().numpy(), want["hit"])
    nef.colors = kept.clone().requires_grad_(True)
    rb = pipe(rays=rays, channels=["rgb"])
    assert len(calls) == before and rb.rgb.requires_grad
    rb.rgb.sum().backward()
    assert float(nef.colors.grad.sum()) == 3.0 * int(want["hit"].sum())
    with torch.no_grad():
        pipe(rays=rays, channels=["rgb"])
    assert len(calls) == before + 1


def test_tracer_handles_batches_without_hits_and_without_rays():
    from wisp.core import Rays
    from wisp.models.nefs import SPCField
    from wisp.tracers import PackedSPCTracer
    tree, level, o, d, colors, _ = _field_inputs()
    nef = SPCField(cuda(tree[0]), dict(colors=cuda(colors)), device=DEV)
    tracer = PackedSPCTracer()
    for fused in (True, False):
        tracer.fused = fused
        rb = tracer(nef, rays=Rays(cuda(o[5:9]), cuda(d[5:9])), channels=["rgb"])
        assert not bool(rb.hit.any()) and float(rb.rgb.abs().sum()) == 0.0 and float(rb.depth.abs().sum()) == 0.0 and float(rb.alpha.sum()) == 0.0
        rb = tracer(nef, rays=Rays(torch.zeros(0, 3, device=DEV), torch.zeros(0, 3, device=DEV)), channels=["rgb"])
        assert rb.rgb.shape == (0, 3) and rb.depth.shape == (0, 1) and rb.hit.shape == (0,) and rb.alpha.shape == (0, 1)


# ------------------------------------------------------------------------------------------------ 7. scripts end to end
def test_mesh2spc_and_render_spc_on_the_procedural_torus(tmp_path, capsys):
    if os.path.join(ROOT, "scripts") not in sys.path:
        sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import render_spc
    from wisp.ops.image import read_png
    out_dir = str(tmp_path / "out")
    record = render_spc.main(["--write-test-mesh", str(tmp_path), "--level", "5", "--num-samples", "200000", "--size", "64", "64",
                              "--out-dir", out_dir, "--device", DEV])
    assert json.loads(capsys.readouterr().out.strip().splitlines()[-1]) == record
    spc = np.load(str(tmp_path / "torus.npz"))
    assert set(spc.files) == {"octree", "colors"} and spc["octree"].dtype == np.uint8 and spc["colors"].dtype == np.uint8
    points, pyramid, exsum = ospc.octree_to_spc(spc["octree"])
    assert pyramid.shape[1] - 2 == 5
    cells = int(pyramid[0, 5])
    assert spc["colors"].shape == (4 * cells,) and record["cells"] == cells and record["rays"] == 4096 and record["level"] == 5
    rgba = spc["colors"].reshape(-1, 4)
    assert bool((rgba[:, 3] == 255).all()) and len(np.unique(rgba[:, :3], axis=0)) > 50          # opaque, really textured
    rays = render_spc.view_rays(64, 64, DEV)
    o, d = rays.origins.cpu().numpy(), rays.dirs.cpu().numpy()
    want_pidx, _, want_hit = ref.first_hit(spc["octree"], points, pyramid, exsum, o, d, 5)
    img = read_png(os.path.join(out_dir, "rgb.png"))
    assert img.shape == (64, 64, 4) and read_png(os.path.join(out_dir, "depth.png")).shape[:2] == (64, 64)
    img = img.reshape(-1, 4)
    assert 300 <= want_hit.sum() < 4096 and abs(record["hit_share"] - want_hit.mean()) < 1e-5
    assert np.array_equal(img[:, 3] == 255, want_hit) and bool((img[~want_hit] == 0).all())
    assert np.array_equal(img[want_hit, :3], rgba[want_pidx[want_hit] - int(pyramid[1, 5]), :3])
