"""GPU: wisp_mesh_closest_tex / wisp_mesh_sample_tex (csrc/mesh_tex.hip) against the reference fixture
tests/golden/mesh_tex_ref.npz (the reference's closest_tex chain executed on the CPU, tests/golden/make_mesh_tex_golden.py) and
against torch's grid_sample on the device; closest_tex with the search included; the textured mesh datasets, NeuralSDFTex under
SDFTrainer and PackedSDFTracer, and scripts/train_sdf_tex.py end to end.

Bounds (tests/mesh_tex_ref.py): hit 1e-12, rgb 1e-4 against the reference.  Every measured value is appended to
profiles/mesh_tex_test_margins.jsonl."""
import importlib.util
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import mesh_tex_ref as ref
from mesh_tex_ref import record

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def golden():
    g = ref.load_golden()
    g["mats"] = ref.mats_from_golden(g)
    d = {k: torch.from_numpy(g[k]).to(DEV) for k in ("vertices", "points", "texv", "hit", "rgb", "dist")}
    d.update({k: torch.from_numpy(g[k]).long().to(DEV) for k in ("faces", "texf", "tidx")})
    d["mesh"] = d["vertices"].double()[d["faces"]].contiguous()
    g["dev"] = d
    return g


@pytest.fixture(scope="module")
def bank(golden):
    from wisp.ops.mesh import TextureBank
    return TextureBank(golden["mats"])


@pytest.fixture(scope="module")
def script():
    spec = importlib.util.spec_from_file_location("train_sdf_tex", os.path.join(ROOT, "scripts", "train_sdf_tex.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def torus_obj(tmp_path_factory, script):
    return script.write_test_mesh(str(tmp_path_factory.mktemp("texmesh")))


@pytest.mark.parametrize("n", [2037, 1, 77])
@pytest.mark.parametrize("as_i64", [False, True])
def test_closest_tex_kernel_matches_the_reference_fixture(golden, bank, n, as_i64):
    import wisp._C as C
    d = golden["dev"]
    sel = slice(2037 - n, 2037)                            # the tail holds the 37 forced Voronoi-region points
    tidx = d["tidx"][sel] if as_i64 else d["tidx"][sel].double()
    hit, rgb = C.mesh_closest_tex(d["points"][sel].double().contiguous(), d["mesh"], tidx.contiguous(), d["texv"], d["texf"],
                                  *bank.to(DEV))
    e_hit, e_rgb = float((hit - d["hit"][sel]).abs().max()), float((rgb - d["rgb"][sel]).abs().max())
    record("gpu_kernel_vs_fixture", n=n, tidx="i64" if as_i64 else "f64", hit=e_hit, rgb=e_rgb, hit_bound=ref.HIT_BOUND,
           rgb_bound=ref.RGB_BOUND)
    assert hit.dtype == torch.float64 and rgb.dtype == torch.float32 and hit.shape == (n, 3) and rgb.shape == (n, 3)
    assert e_hit <= ref.HIT_BOUND and e_rgb <= ref.RGB_BOUND
    # and against the operation-for-operation restatement on the host
    want_hit, want_rgb, _ = ref.closest_tex_ref(d["points"][sel].cpu(), d["mesh"].cpu(), d["tidx"][sel].cpu(), d["texv"].cpu(),
                                                d["texf"].cpu(), golden["mats"])
    # (the same operations; only the reflection's x - flips * span may be fused on the device: <= 1 ulp(15) = 9.5e-7 of a texel per axis)
    assert float((hit.cpu() - want_hit).abs().max()) <= 1e-15 and float((rgb.cpu() - want_rgb).abs().max()) <= 4e-6


def test_closest_tex_with_the_search_matches_the_fixture_for_every_split(golden, bank):
    from wisp.ops.mesh import closest_point, closest_tex, compute_sdf
    d = golden["dev"]
    uniq = torch.from_numpy(golden["unique"]).to(DEV)
    pts = d["points"][uniq]
    assert pts.shape == (2000, 3)
    _, _, tidx = closest_point(d["vertices"], d["faces"], pts)
    assert torch.equal(tidx, d["tidx"][uniq])
    outs = [closest_tex(d["vertices"], d["faces"], d["texv"], d["texf"], bank, pts, split_size=s) for s in (2000, 512, 1)]
    rgb, hit, dist = outs[0]
    assert rgb.dtype == torch.float32 and rgb.shape == (2000, 3) and hit.shape == (2000, 3) and dist.shape == (2000,)
    assert torch.equal(dist, compute_sdf(d["vertices"], d["faces"], pts)[:, 0])                  # bitwise
    e_rgb, e_hit = float((rgb - d["rgb"][uniq]).abs().max()), float((hit - d["hit"][uniq]).abs().max())
    e_dist = float((dist - d["dist"][uniq]).abs().max())
    record("gpu_closest_tex_vs_fixture", rgb=e_rgb, hit=e_hit, dist=e_dist, rgb_bound=ref.RGB_BOUND, hit_bound=ref.HIT_BOUND)
    assert e_rgb <= ref.RGB_BOUND and e_hit <= ref.HIT_BOUND
    for other in outs[1:]:
        assert all(torch.equal(a, b) for a, b in zip(outs[0], other))
    from_dict = closest_tex(d["vertices"], d["faces"], d["texv"].cpu(), d["texf"].cpu(), golden["mats"], pts.cpu())
    assert all(torch.equal(a, b) for a, b in zip(outs[0], from_dict))       # the materials dict, host inputs moved to V's device
    empty = closest_tex(d["vertices"], d["faces"], d["texv"], d["texf"], bank, pts[:0])
    assert empty[0].shape == (0, 3) and empty[1].shape == (0, 3) and empty[2].shape == (0,)


def test_colour_identities(golden, bank):
    import wisp._C as C
    from wisp.ops.mesh import sample_tex
    d = golden["dev"]
    material = d["texf"][d["tidx"], 3]
    pts = d["points"].double().contiguous()
    _, rgb = C.mesh_closest_tex(pts, d["mesh"], d["tidx"], d["texv"], d["texf"], *bank.to(DEV))
    kd = golden["mats"][1]['diffuse'].to(DEV)
    assert int((material == 1).sum()) > 100 and torch.equal(rgb[material == 1], kd.expand(int((material == 1).sum()), 3))
    assert int((material == -1).sum()) > 100 and not rgb[material == -1].any()
    none = torch.full_like(d["tidx"], -1)
    hit, rgb = C.mesh_closest_tex(pts, d["mesh"], none, d["texv"], d["texf"], *bank.to(DEV))
    assert not rgb.any()
    from wisp.ops.mesh import closest_point_on_triangle
    assert float((hit - closest_point_on_triangle(d["mesh"][:1].expand(pts.shape[0], 3, 3), pts)).abs().max()) <= 1e-15
    _, rgb = C.mesh_closest_tex(pts, d["mesh"], none.double(), d["texv"], d["texf"], *bank.to(DEV))
    assert not rgb.any()
    # an id without a record, and a texture-vertex index outside texv on a mapped material
    texf = d["texf"].clone()
    texf[:, 3] = 7
    assert not C.mesh_closest_tex(pts, d["mesh"], d["tidx"], d["texv"], texf, *bank.to(DEV))[1].any()
    texf = d["texf"].clone()
    texf[:, 0] = d["texv"].shape[0]
    rgb = C.mesh_closest_tex(pts, d["mesh"], d["tidx"], d["texv"], texf, *bank.to(DEV))[1]
    assert not rgb[(material == 0) | (material == 2)].any() and torch.equal(rgb[material == 1][0], kd)
    # texel centres
    worst = 0.0
    for i in (0, 2):
        tex = golden["mats"][i]['diffuse_texname'][..., :3].to(DEV)
        h, w = tex.shape[:2]
        ys, xs = torch.meshgrid(torch.arange(h, device=DEV), torch.arange(w, device=DEV), indexing='ij')
        u = xs.float() / (w - 1) if w > 1 else torch.full_like(xs, 0.37, dtype=torch.float32)
        v = 1.0 - ys.float() / (h - 1) if h > 1 else torch.full_like(ys, 0.37, dtype=torch.float32)
        got = sample_tex(torch.stack([u, v], -1).reshape(-1, 2), torch.full((h * w,), i, device=DEV), bank)
        worst = max(worst, float((got - tex.reshape(-1, 3)).abs().max()))
    record("gpu_sample_tex_texel_centres", err=worst, bound=1e-6)
    assert worst <= 1e-6
    assert not sample_tex(torch.rand(5, 2, device=DEV), torch.tensor([-1, 3, 99, -7, 1 << 40], device=DEV), bank).any()
    assert sample_tex(torch.zeros(0, 2, device=DEV), torch.zeros(0, dtype=torch.int64, device=DEV), bank).shape == (0, 3)


def test_sample_tex_is_grid_sample(golden, bank):
    from wisp.ops.mesh import sample_tex
    g = torch.Generator(device=DEV).manual_seed(9)
    worst = {}
    for i in (0, 2):
        tex = golden["mats"][i]['diffuse_texname'].to(DEV)
        uv = torch.rand(4096, 2, device=DEV, generator=g) * 7 - 3
        grid = torch.stack([uv[:, 0] * 2 - 1, -(uv[:, 1] * 2 - 1)], -1).reshape(1, -1, 1, 2)
        want = torch.nn.functional.grid_sample(tex[..., :3].permute(2, 0, 1)[None], grid, mode='bilinear', padding_mode='reflection',
                                               align_corners=True)[0, :, :, 0].T
        got = sample_tex(uv, torch.full((4096,), i, device=DEV), golden["mats"] if i else bank)
        worst[f"map{i}"] = float((got - want).abs().max())
    record("gpu_sample_tex_vs_grid_sample", bound=1e-5, **worst)
    assert max(worst.values()) <= 1e-5
    mixed = torch.arange(4096, device=DEV) % 4 - 1                      # -1, 0, 1, 2 interleaved: one launch for all materials
    got = sample_tex(uv, mixed, bank)
    for i in (0, 2):
        assert torch.equal(got[mixed == i], sample_tex(uv[mixed == i], mixed[mixed == i], bank))
    assert not got[mixed == -1].any() and torch.equal(got[mixed == 1][0], golden["mats"][1]['diffuse'].to(DEV))


def _check_textured(ds, compute_sdf, V, F):
    rgb, sdf, coords = ds.data['rgb'], ds.data['sdf'], ds.data['coords']
    m = coords.shape[0]
    assert rgb.dtype == torch.float32 and rgb.shape == (m, 3) and rgb.is_cuda
    assert float(rgb.min()) >= 0.0 and float(rgb.max()) <= 1.0 and float(rgb.std()) > 0.05
    assert sdf.shape == (m, 1) and torch.equal(sdf, compute_sdf(V, F, coords))
    b = ds.get_batch(torch.arange(0, m, 7, device=DEV))
    assert torch.equal(b['rgb'], rgb[::7]) and torch.equal(b['sdf'], sdf[::7]) and b['coords'].shape[0] == b['rgb'].shape[0]


def test_textured_datasets_on_a_torus(torus_obj):
    from wisp.accelstructs import OctreeAS
    from wisp.datasets import MeshSampledSDFDataset, OctreeSampledSDFDataset
    from wisp.ops.mesh import TextureBank, compute_sdf
    torch.manual_seed(3)
    blas = OctreeAS.from_mesh(torus_obj, level=5, sample_tex=True, num_samples_on_mesh=500_000)
    ext = blas.extent
    assert ext['texv'].shape == (49 * 25, 2) and ext['texv'].dtype == torch.float32
    assert ext['texf'].shape == (2 * 48 * 24, 4) and ext['texf'].dtype == torch.int64 and ext['faces'].shape == (2 * 48 * 24, 3)
    assert sorted(ext['mats']) == [0, 1, 2] and ext['mats'][0]['diffuse_texname'].shape == (64, 128, 3)
    assert 'diffuse_texname' not in ext['mats'][1] and ext['mats'][2]['diffuse_texname'].shape == (32, 32, 4)
    assert isinstance(ext['tex_bank'], TextureBank)
    ods = OctreeSampledSDFDataset(blas, split='train', sample_tex=True, samples_per_voxel=4, num_samples=5000)
    assert len(ods) == 5000 and ods.data_pool['rgb'].shape == (ods.pool_size, 3)
    _check_textured(ods, compute_sdf, ext['vertices'], ext['faces'])
    mds = MeshSampledSDFDataset(torus_obj, split='train', sample_tex=True, num_samples=1000)
    assert len(mds) == 5000 and mds.tex_bank is not None and sorted(mds.mats) == [0, 1, 2]
    _check_textured(mds, compute_sdf, mds.verts, mds.faces)
    bank_before = mds.tex_bank
    for ds in (ods, mds):
        before = ds.data['rgb'].clone()
        ds.resample()
        assert not torch.equal(ds.data['rgb'], before)
        _check_textured(ds, compute_sdf, ext['vertices'] if ds is ods else mds.verts, ext['faces'] if ds is ods else mds.faces)
    assert mds.tex_bank is bank_before and blas.extent['tex_bank'] is ext['tex_bank']     # resample() does not rebuild the bank
    # the plain-diffuse third of the tube carries exactly its Kd
    on = mds.data['coords'][4000:]                                   # 'trace' samples lie on the surface
    assert bool((mds.data['rgb'][4000:] == torch.tensor([0.2, 0.4, 0.8], device=DEV)).all(dim=1).any()) and on.shape[0] == 1000


def test_sdf_tex_training_and_tracing(torus_obj, script):
    from wisp.accelstructs import OctreeAS
    from wisp.datasets import OctreeSampledSDFDataset
    from wisp.models import Pipeline
    from wisp.models.grids import OctreeGrid
    from wisp.models.nefs import NeuralSDFTex
    from wisp.tracers import PackedSDFTracer
    from wisp.trainers import SDFTrainer, ConfigSDFTrainer, ConfigAdam, ConfigDataloader
    torch.manual_seed(2)
    blas = OctreeAS.from_mesh(torus_obj, level=5, sample_tex=True, num_samples_on_mesh=1_000_000)
    ods = OctreeSampledSDFDataset(blas, split='train', sample_tex=True, samples_per_voxel=8, num_samples=30000)
    grid = OctreeGrid(blas, feature_dim=16, num_lods=3, multiscale_type='sum', feature_std=0.05)
    nef = NeuralSDFTex(grid, embedder_type='identity', hidden_dim=128, num_layers=1).to(DEV)
    history = []

    class Trainer(SDFTrainer):
        def log_console(self):
            m = self.tracker.metrics
            history.append((m.average_metric('l2_loss'), m.average_metric('rgb_loss')))

    cfg = ConfigSDFTrainer(optimizer=ConfigAdam(lr=1e-3, eps=1e-15), dataloader=ConfigDataloader(batch_size=512), max_epochs=3,
                           resample=True, profile_nvtx=False)
    tr = Trainer(cfg, Pipeline(nef, None), ods, device=DEV)
    tr.train()
    assert len(history) == 3 and np.isfinite(history).all()
    (l2_first, rgb_first), (l2_last, rgb_last) = history[0], history[-1]
    record("gpu_sdf_tex_training", l2_first=l2_first, l2_last=l2_last, rgb_first=rgb_first, rgb_last=rgb_last,
           l2_ratio=l2_last / l2_first, rgb_ratio=rgb_last / rgb_first)
    assert rgb_last < rgb_first and l2_last < l2_first
    tracer = PackedSDFTracer(num_steps=48, step_size=0.8, min_dis=0.0003)
    with torch.no_grad():
        rb = tracer(nef, rays=script.view_rays(48, 48, DEV), channels=["depth", "hit"], lod_idx=None)
        hit = rb.hit.reshape(-1)
        assert 100 < int(hit.sum()) < 48 * 48
        xyz = rb.xyz.reshape(-1, 3)[hit]
        rgb = nef(coords=xyz, channels="rgb")
    assert rgb.shape == (int(hit.sum()), 3) and float(rgb.min()) >= 0.0 and float(rgb.max()) <= 1.0
    rho = torch.hypot(torch.hypot(xyz[:, 0], xyz[:, 1]) - 0.6 / 0.85, xyz[:, 2])       # the torus after sphere normalisation
    assert float((rho - 0.25 / 0.85).abs().median()) < 0.05


def test_train_sdf_tex_script_runs_end_to_end(tmp_path):
    out = tmp_path / "out"
    cmd = [sys.executable, os.path.join(ROOT, "scripts", "train_sdf_tex.py"), "--write-test-mesh", str(tmp_path / "mesh"), "--epochs", "2",
           "--level", "5", "--num-samples", "20000", "--mesh-samples", "500000", "--size", "48", "48", "--out-dir", str(out)]
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-4000:]
    rec = json.loads(res.stdout.strip().splitlines()[-1])
    assert os.path.isfile(out / "albedo.png") and rec["albedo"] == str(out / "albedo.png")
    from wisp.ops.image.io import load_u8
    img = load_u8(str(out / "albedo.png"))
    assert img.shape == (48, 48, 3) and rec["hits"] > 100 and int((img != 255).any(axis=2).sum()) > 100
    assert os.path.isfile(tmp_path / "mesh" / "torus.obj") and os.path.isfile(tmp_path / "mesh" / "stripes.png")
    record("gpu_train_sdf_tex_script", **{k: rec[k] for k in ("hits", "seconds", "l2_first", "l2_last", "rgb_first", "rgb_last")})
