"""CPU: the restatement of the texture kernels (tests/mesh_tex_ref.py) against the reference fixture and against the reference
chain executed in place; load_obj(load_materials=True) on a hand-written OBJ + MTL + PNGs; NeuralSDFTex against the reference
class executed in place; the errors of the textured paths that need no device; resources of the texture kernels.

Measured (profiles/mesh_tex_test_margins.jsonl): restatement against the fixture, hit 1.1e-16 (bound 1e-12), rgb 2.1e-6
(bound 1e-4)."""
import os
import sys
import types

import numpy as np
import pytest
import torch

import kernel_meta
import mesh_sdf_oracle as oracle
import mesh_tex_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "kaolin-wisp_amd", "csrc", "libwisp_hip.so")
record = ref.record


@pytest.fixture(scope="module")
def golden():
    g = ref.load_golden()
    g["mats"] = ref.mats_from_golden(g)
    g["mesh"] = torch.from_numpy(g["vertices"]).double()[torch.from_numpy(g["faces"]).long()]
    return g


def test_fixture_is_the_scene_this_tree_builds(golden):
    V, F, texv, texf, mats = ref.scene()
    assert np.array_equal(golden["vertices"], V.astype(np.float32)) and np.array_equal(golden["faces"], F)
    assert np.array_equal(golden["texv"], texv) and np.array_equal(golden["texf"], texf)
    assert torch.equal(golden["mats"][0]['diffuse_texname'], mats[0]['diffuse_texname']) and golden["map0"].shape == (5, 9, 3)
    assert torch.equal(golden["mats"][2]['diffuse_texname'], mats[2]['diffuse_texname']) and golden["map2"].shape == (16, 1, 4)
    assert golden["points"].shape == (2037, 3) and int(golden["unique"].sum()) == 2000
    _, region = ref.closest_point_and_region(golden["mesh"][torch.from_numpy(golden["tidx"][-37:]).long()],
                                             torch.from_numpy(golden["points"][-37:]).double())
    assert sorted(set(region.tolist())) == list(range(7))                 # every Voronoi region is taken


def test_restated_kernel_arithmetic_matches_the_reference_fixture(golden):
    hit, rgb, _ = ref.closest_tex_ref(torch.from_numpy(golden["points"]), golden["mesh"], torch.from_numpy(golden["tidx"]),
                                      torch.from_numpy(golden["texv"]), torch.from_numpy(golden["texf"]).long(), golden["mats"])
    e_hit = np.abs(hit.numpy() - golden["hit"]).max()
    e_rgb = np.abs(rgb.numpy() - golden["rgb"]).max()
    record("host_restatement_vs_fixture", hit=e_hit, rgb=e_rgb, hit_bound=ref.HIT_BOUND, rgb_bound=ref.RGB_BOUND)
    assert e_hit <= ref.HIT_BOUND and e_rgb <= ref.RGB_BOUND
    assert rgb.dtype == torch.float32 and hit.dtype == torch.float64
    kd_only = torch.from_numpy(golden["texf"][golden["tidx"], 3] == 1)
    assert torch.equal(rgb[kd_only], golden["mats"][1]['diffuse'].expand(int(kd_only.sum()), 3))       # bit for bit
    assert not rgb[torch.from_numpy(golden["texf"][golden["tidx"], 3] == -1)].any()


@pytest.mark.skipif(not ref.have_reference(), reason="reference tree absent")
def test_restated_kernel_arithmetic_matches_the_reference_in_place(golden):
    n = 300
    pts = np.concatenate([golden["points"][:n], golden["points"][-37:]])
    forced = golden["tidx"][-37:]
    rgb, hit, dist, tidx = ref.reference_closest_tex(torch.from_numpy(golden["vertices"]), torch.from_numpy(golden["faces"]).long(),
                                                     torch.from_numpy(golden["texv"]), torch.from_numpy(golden["texf"]).long(),
                                                     golden["mats"], torch.from_numpy(pts), forced_tidx=forced)
    sel = np.r_[0:n, 2000:2037]
    assert np.array_equal(tidx.numpy(), golden["tidx"][sel]) and np.array_equal(rgb.numpy(), golden["rgb"][sel])
    mine_hit, mine_rgb, _ = ref.closest_tex_ref(torch.from_numpy(pts), golden["mesh"], tidx, torch.from_numpy(golden["texv"]),
                                                torch.from_numpy(golden["texf"]).long(), golden["mats"])
    assert float((mine_hit - hit).abs().max()) <= ref.HIT_BOUND and float((mine_rgb - rgb).abs().max()) <= ref.RGB_BOUND


def test_restated_sample_tex_is_grid_sample_on_the_host(golden):
    g = torch.Generator().manual_seed(5)
    for i in (0, 2):
        tex = golden["mats"][i]['diffuse_texname']
        uv = torch.rand(4096, 2, generator=g) * 7 - 3
        grid = torch.stack([uv[:, 0] * 2 - 1, -(uv[:, 1] * 2 - 1)], -1).reshape(1, -1, 1, 2)
        want = torch.nn.functional.grid_sample(tex[..., :3].permute(2, 0, 1)[None], grid, mode='bilinear', padding_mode='reflection',
                                               align_corners=True)[0, :, :, 0].T
        got = ref.sample_tex_ref(uv, torch.full((4096,), i), golden["mats"])
        assert float((got - want).abs().max()) <= 1e-5


# ------------------------------------------------------------------------------------------------ load_obj with materials
def _write_scene(tmp_path, mtl_extra="", face_extra=""):
    from wisp.ops.image.io import write_png
    rng = np.random.default_rng(7)
    rgb, rgba = rng.integers(0, 256, (3, 4, 3), dtype=np.uint8), rng.integers(0, 256, (2, 2, 4), dtype=np.uint8)
    write_png(str(tmp_path / "wood.png"), rgb)
    os.makedirs(tmp_path / "tex", exist_ok=True)
    write_png(str(tmp_path / "tex" / "paint.png"), rgba)
    (tmp_path / "scene.mtl").write_text("# two materials\nnewmtl wood\nKd 0.5 0.25 0.125\nmap_Kd wood.png\n\nnewmtl paint\nNs 10\n"
                                        "map_Kd tex/paint.png\n" + mtl_extra)
    (tmp_path / "scene.obj").write_text(
        "mtllib scene.mtl\n"
        "v 0 0 0\nv 1 0 0\nv 1 1 0\nv 0 1 0\nv 2 0 0\nv 2 1 0\nv 1.5 2 0\nv 0 0 1\n"
        "vt 0 0\nvt 1 0\nvt 1 1\nvt 0 1\nvt 0.5 2.5\n"
        "vn 0 0 1\n"
        "f 1 2 3\n"                                    # before any usemtl: material -1, no texcoords
        "f 1//1 2//1 8//1\n"
        "usemtl wood\n"
        "f 1/1 2/2 3/3 4/4\n"                          # a quad
        "usemtl paint\n"
        "f 2/2/1 5/1/1 6/4/1 7/-1/1 3/3/1\n"           # a pentagon, one relative vt index
        + face_extra)
    return str(tmp_path / "scene.obj"), rgb, rgba


def test_load_obj_with_materials_on_a_hand_written_scene(tmp_path):
    from wisp.ops.mesh import load_obj
    path, rgb, rgba = _write_scene(tmp_path)
    V, F, texv, texf, mats = load_obj(path, load_materials=True)
    assert V.dtype == torch.float32 and V.shape == (8, 3)
    assert F.tolist() == [[0, 1, 2], [0, 1, 7], [0, 1, 2], [0, 2, 3], [1, 4, 5], [1, 5, 6], [1, 6, 2]]
    assert texv.dtype == torch.float32 and texv.tolist() == [[0, 0], [1, 0], [1, 1], [0, 1], [0.5, 2.5]]
    assert texf.dtype == torch.int64 and texf.tolist() == [[-1, -1, -1, -1], [-1, -1, -1, -1], [0, 1, 2, 0], [0, 2, 3, 0],
                                                           [1, 0, 3, 1], [1, 3, 4, 1], [1, 4, 2, 1]]
    assert sorted(mats) == [0, 1] and sorted(mats[0]) == ['diffuse', 'diffuse_texname'] == sorted(mats[1])
    assert torch.equal(mats[0]['diffuse'], torch.tensor([0.5, 0.25, 0.125])) and torch.equal(mats[1]['diffuse'], torch.zeros(3))
    assert torch.equal(mats[0]['diffuse_texname'], torch.from_numpy(rgb.astype(np.float32) / np.float32(255)))
    assert mats[1]['diffuse_texname'].shape == (2, 2, 4)
    assert torch.equal(mats[1]['diffuse_texname'], torch.from_numpy(rgba.astype(np.float32) / np.float32(255)))
    V2, F2 = load_obj(path)                                        # the plain call is unchanged
    assert torch.equal(V2, V) and torch.equal(F2, F)
    assert len(load_obj(path, load_materials=False)) == 2


def test_load_obj_with_materials_refuses_what_it_cannot_read(tmp_path):
    from wisp.ops.image.io import write_png
    from wisp.ops.mesh import load_obj
    a, b, c = tmp_path / "a", tmp_path / "b", tmp_path / "c"
    for d in (a, b, c):
        d.mkdir()
    write_png(str(a / "grey.png"), np.zeros((4, 3), dtype=np.uint8))
    path, _, _ = _write_scene(a, mtl_extra="newmtl grey\nmap_Kd grey.png\n")
    with pytest.raises(ValueError, match="3 or 4 channels"):
        load_obj(path, load_materials=True)
    path, _, _ = _write_scene(b, mtl_extra="newmtl scaled\nmap_Kd -s 2 2 1 wood.png\n")
    with pytest.raises(ValueError, match="options"):
        load_obj(path, load_materials=True)
    path, _, _ = _write_scene(c, face_extra="usemtl wood\nf 1 2 3\n")
    with pytest.raises(ValueError, match="texture coordinate"):
        load_obj(path, load_materials=True)
    assert len(load_obj(path)) == 2                                # geometry alone still loads


def test_load_obj_without_materials_returns_empties(tmp_path):
    from wisp.ops.mesh import load_obj
    obj = oracle.write_obj(tmp_path / "tri.obj", *oracle.single_triangle())
    V, F, texv, texf, mats = load_obj(obj, load_materials=True)
    assert V.shape == (3, 3) and F.tolist() == [[0, 1, 2]]
    assert texv.shape == (0, 2) and texv.dtype == torch.float32 and texf.tolist() == [[-1, -1, -1, -1]] and mats == {}


def test_texture_bank_layout():
    import ctypes
    import wisp._C as C
    from wisp.ops.mesh import TextureBank
    assert ctypes.sizeof(C.TexMaterial) == 32
    g = ref.load_golden()
    bank = TextureBank(ref.mats_from_golden(g))
    assert bank.texels.shape == (5 * 9 + 16, 3) and bank.texels.dtype == torch.float32 and bank.num_materials == 3
    assert torch.equal(bank.texels[:45], torch.from_numpy(g["map0"]).reshape(-1, 3))
    assert torch.equal(bank.texels[45:], torch.from_numpy(g["map2"][..., :3]).reshape(-1, 3))
    recs = (C.TexMaterial * 3).from_buffer_copy(bank.records.numpy().tobytes())
    assert [(r.offset, r.height, r.width, r.has_map) for r in recs] == [(0, 5, 9, 1), (0, 0, 0, 0), (45, 16, 1, 1)]
    assert list(recs[1].kd) == [0.25, 0.5, 0.75]
    sparse = TextureBank({2: {'diffuse': torch.tensor([1.0, 0.0, 0.5])}})          # ids 0 and 1 have no record of their own
    assert sparse.num_materials == 3 and sparse.texels.shape == (0, 3)
    assert TextureBank({}).num_materials == 0
    with pytest.raises(ValueError):
        TextureBank({0: {'diffuse_texname': torch.zeros(4, 4)}})


# ------------------------------------------------------------------------------------------------ NeuralSDFTex
REFW = os.path.join(ref.REF, "wisp")


def _exec_reference_module(rel):
    path = os.path.join(REFW, rel)
    name = "reference_" + rel.replace("/", "_").replace(".py", "")
    mod = types.ModuleType(name)
    mod.__file__ = path
    sys.modules[name] = mod
    exec(compile(open(path).read(), path, "exec"), mod.__dict__)
    return mod.__dict__


class _StandInGrid(torch.nn.Module):
    """A CPU grid with the attributes the field reads: interpolate() is a fixed smooth function of the coordinates and a table."""

    def __init__(self, feature_dim=6, num_lods=3, multiscale_type='sum'):
        super().__init__()
        self.feature_dim, self.num_lods, self.multiscale_type = feature_dim, num_lods, multiscale_type
        width = feature_dim * num_lods if multiscale_type == 'cat' else feature_dim
        self.table = torch.nn.Parameter(torch.randn(3, width) * 0.3)

    def interpolate(self, coords, lod_idx):
        return torch.sin(coords * (lod_idx + 1.0)) @ self.table


@pytest.mark.skipif(not os.path.isfile(os.path.join(REFW, "models/nefs/neural_sdf_tex.py")), reason="reference tree absent")
@pytest.mark.parametrize("kw", [dict(), dict(embedder_type='positional', pos_multires=4, hidden_dim=32, num_layers=2),
                                dict(embedder_type='identity', activation_type='relu', hidden_dim=16)])
def test_neural_sdf_tex_equals_the_reference_class(kw):
    """The reference's own NeuralSDFTex (models/nefs/neural_sdf_tex.py:20-123) executed in place.  Two names it reads do not exist
    in its own tree and are supplied here, which is what the package class states as its differences: the `active` keyword of
    get_positional_embedder (:59; the factory took it when the class was written: inactive = identity of width 3), and
    `self.num_lods` (:66, :102), set from the grid."""
    from wisp.models.embedders import get_positional_embedder
    from wisp.models.nefs import NeuralSDFTex as Mine
    ns = _exec_reference_module("models/nefs/neural_sdf_tex.py")
    ns["get_positional_embedder"] = lambda frequencies, active, input_dim=3: \
        get_positional_embedder(frequencies, input_dim=input_dim) if active else (torch.nn.Identity(), input_dim)
    Ref = ns["NeuralSDFTex"]
    for multiscale in ('sum',):
        torch.manual_seed(4)
        r = Ref(_StandInGrid(multiscale_type=multiscale), **kw)
        torch.manual_seed(4)
        m = Mine(_StandInGrid(multiscale_type=multiscale), **kw)
        r.num_lods = r.grid.num_lods
        rs, ms = r.state_dict(), m.state_dict()
        assert list(rs) == list(ms)
        for k in rs:
            assert rs[k].shape == ms[k].shape and rs[k].dtype == ms[k].dtype and torch.equal(rs[k], ms[k]), k
        for attr in ("embedder_type", "pos_multires", "pos_embed_dim", "activation_type", "layer_type", "hidden_dim", "num_layers",
                     "position_input", "effective_feature_dim", "input_dim"):
            assert getattr(r, attr) == getattr(m, attr), attr
        assert r.get_supported_channels() == m.get_supported_channels() == {"rgb", "sdf"}
        assert m.decoder.lout.out_features == 4
        g = torch.Generator().manual_seed(6)
        for shape in ((17, 3), (5, 4, 3), (0, 3), (0, 2, 3)):
            x = torch.rand(*shape, generator=g) * 2 - 1
            if kw.get('embedder_type') == 'positional' and shape[0]:
                want = None                     # the embedder takes [N, 3] and the reference hands it [N, S, 3]: it cannot run
            else:
                want = r.rgbsdf(x, lod_idx=1)
            got = m.rgbsdf(x, lod_idx=1)
            assert got["rgb"].shape == (*shape[:-1], 3) and got["sdf"].shape == (*shape[:-1], 1)
            if want is not None:
                assert torch.equal(got["rgb"], want["rgb"]) and torch.equal(got["sdf"], want["sdf"]), shape
            if shape[0]:
                assert torch.equal(m.rgbsdf(x)["sdf"], m.rgbsdf(x, lod_idx=2)["sdf"])        # None = the grid's finest LOD
                c, d = m(coords=x, lod_idx=1, channels=["rgb", "sdf"])
                assert torch.equal(c, got["rgb"]) and torch.equal(d, got["sdf"])
                assert float(c.detach().min()) >= 0 and float(c.detach().max()) <= 1
    cat = Mine(_StandInGrid(multiscale_type='cat'))
    assert cat.effective_feature_dim == 18 and cat.input_dim == 18


def test_neural_sdf_tex_without_the_reference():
    from wisp.models.nefs import NeuralSDFTex
    torch.manual_seed(1)
    nef = NeuralSDFTex(_StandInGrid(), embedder_type='positional', pos_multires=2, hidden_dim=8)
    assert nef.pos_embed_dim == 15 and nef.input_dim == 21 and nef.get_supported_channels() == {"rgb", "sdf"}
    out = nef.rgbsdf(torch.rand(4, 2, 3))
    assert out["rgb"].shape == (4, 2, 3) and out["sdf"].shape == (4, 2, 1)
    assert nef.rgbsdf(torch.zeros(0, 3))["sdf"].shape == (0, 1)
    out["sdf"].sum().backward()
    assert nef.grid.table.grad is not None and nef.decoder.lout.weight.grad is not None


# ------------------------------------------------------------------------------------------------ errors without a device
def test_textured_paths_refuse_what_has_no_materials_without_a_device(tmp_path):
    from wisp.accelstructs import OctreeAS
    from wisp.datasets import MeshSampledSDFDataset, OctreeSampledSDFDataset
    obj = oracle.write_obj(tmp_path / "tri.obj", *oracle.single_triangle())
    with pytest.raises(NotImplementedError, match="no materials"):
        MeshSampledSDFDataset(obj, split='train', sample_tex=True)
    with pytest.raises(NotImplementedError, match="no materials"):
        OctreeAS.from_mesh(obj, level=3, sample_tex=True)
    fake = OctreeAS.make_dense(2)
    fake.extent['vertices'], fake.extent['faces'] = torch.zeros(3, 3), torch.zeros(1, 3, dtype=torch.long)
    with pytest.raises(NotImplementedError, match="no materials"):
        OctreeSampledSDFDataset(fake, split='train', sample_tex=True)
    fake.extent['mats'] = {}                                    # an empty dict is no material either
    fake.extent['texv'], fake.extent['texf'] = torch.zeros(0, 2), torch.full((1, 4), -1)
    with pytest.raises(NotImplementedError, match="no materials"):
        OctreeSampledSDFDataset(fake, split='train', sample_tex=True)


def test_texture_ops_refuse_cpu_tensors(golden):
    from wisp.ops.mesh import closest_tex, sample_tex
    with pytest.raises(RuntimeError, match="GPU tensor"):
        sample_tex(torch.zeros(4, 2), torch.zeros(4, dtype=torch.int64), golden["mats"])
    with pytest.raises(RuntimeError, match="GPU tensor"):
        closest_tex(torch.from_numpy(golden["vertices"]), torch.from_numpy(golden["faces"]).long(), torch.from_numpy(golden["texv"]),
                    torch.from_numpy(golden["texf"]).long(), golden["mats"], torch.zeros(4, 3))


@pytest.mark.skipif(not kernel_meta.available(LIB), reason="libwisp_hip.so not built or llvm-readelf missing")
def test_mesh_tex_kernels_have_zero_scratch_and_allowed_workgroups():
    meta = kernel_meta.kernels(LIB)
    names = kernel_meta.demangled(list(meta))
    ours = {names[k]: v for k, v in meta.items() if "mesh_tex_" in names[k]}
    assert len(ours) == 3, sorted(ours)                  # closest (f64 / i64 triangle index), sample
    for name, v in ours.items():
        assert "mesh_sdf_" not in name
        assert v["scratch"] == 0 and v["wg"] in (64, 128, 256, 512, 1024), (name, v)
