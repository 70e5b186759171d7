"""CPU: the mesh -> SDF oracle (tests/mesh_sdf_oracle.py) against analytic signed distances and against the reference's own
closest_point_on_triangle / sample_spc executed in place; the package's closest_point_on_triangle and sample_spc; validation and
constructor schemas of the mesh-sampled SDF datasets; resources of the mesh SDF kernels."""
import inspect
import os
import re

import numpy as np
import pytest
import torch

import kernel_meta
import mesh_sdf_oracle as oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "kaolin-wisp_amd", "csrc", "libwisp_hip.so")
REF = "/root/reference"


def _exec_reference(relpath, names):
    """Run a reference source file in place (never copied) and return the named functions."""
    path = os.path.join(REF, relpath)
    src = open(path).read()
    src = re.sub(r"^import wisp\._C as _C\s*$", "", src, flags=re.M)
    ns = {"__name__": "reference_" + os.path.basename(path)}
    exec(compile(src, path, "exec"), ns)
    return [ns[n] for n in names]


def test_oracle_box_is_the_analytic_box_sdf():
    V, F = oracle.box(0.5)
    rng = np.random.default_rng(1)
    P = np.concatenate([rng.uniform(-1.2, 1.2, (600, 3)), rng.uniform(-0.5, 0.5, (200, 3))])
    sdf, idx, amb, _ = oracle.mesh_sdf(P, V[F])
    want = oracle.box_sdf(P)
    assert np.all(np.abs(np.abs(sdf) - np.abs(want)) <= 3e-7 * np.abs(want) + 1e-7)
    off = np.abs(want) > 1e-6
    assert np.array_equal(np.sign(sdf[off]), np.sign(want[off])) and amb.mean() < 1e-3
    assert idx.min() >= 0 and idx.max() < 12


@pytest.mark.parametrize("which", ["icosphere", "bumpy"])
def test_oracle_sign_and_faceting_bound_on_spheres(which):
    rng = np.random.default_rng(2)
    P = rng.uniform(-1.0, 1.0, (300, 3))
    r = np.linalg.norm(P, axis=1)
    if which == "icosphere":
        V, F = oracle.icosphere(3)
        true_r, bound = np.ones_like(r), 0.01
    else:
        V, F = oracle.bumpy_sphere(3)
        true_r, bound = oracle.bumpy_radius(P / r[:, None]), 0.03
    sdf, _, amb, _ = oracle.mesh_sdf(P, V[F])
    off = np.abs(r - true_r) > bound
    assert np.array_equal(sdf[off] < 0, (r < true_r)[off]) and amb.mean() < 1e-3
    if which == "icosphere":
        assert np.all(np.abs(np.abs(sdf) - np.abs(r - 1)) <= bound)


def _voronoi_cases():
    """A fixed triangle and points in each of its seven Voronoi regions (3 vertices, 3 edges, the face), off its plane too."""
    tri = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.2, 0.9, 0.0]])
    P = np.array([[-0.3, -0.2, 0.1], [1.4, -0.2, -0.3], [0.1, 1.3, 0.2],      # vertices a, b, c
                  [0.5, -0.4, 0.2], [0.8, 0.7, -0.1], [-0.3, 0.5, 0.4],       # edges ab, bc, ca
                  [0.4, 0.3, 0.5], [0.3, 0.2, -0.7]])                         # face
    rng = np.random.default_rng(3)
    T = np.concatenate([np.repeat(tri[None], len(P), 0), rng.normal(size=(200, 3, 3))])
    P = np.concatenate([P, rng.normal(size=(200, 3)) * 1.5])
    return T, P


def test_package_closest_point_on_triangle_matches_the_oracle():
    from wisp.ops.mesh import closest_point_on_triangle
    T, P = _voronoi_cases()
    got = closest_point_on_triangle(torch.from_numpy(T), torch.from_numpy(P)).numpy()
    assert np.allclose(got, oracle.closest_point_on_triangle(T, P), atol=1e-12)


@pytest.mark.skipif(not os.path.isfile(os.path.join(REF, "wisp/ops/mesh/closest_point.py")), reason="reference tree absent")
def test_closest_point_on_triangle_matches_reference():
    from wisp.ops.mesh import closest_point_on_triangle
    ref, = _exec_reference("wisp/ops/mesh/closest_point.py", ["closest_point_on_triangle"])
    T, P = _voronoi_cases()
    want = ref(torch.from_numpy(T), torch.from_numpy(P)).numpy()
    assert np.allclose(oracle.closest_point_on_triangle(T, P), want, atol=1e-12)
    assert np.allclose(closest_point_on_triangle(torch.from_numpy(T), torch.from_numpy(P)).numpy(), want, rtol=0, atol=1e-14)


@pytest.mark.skipif(not os.path.isfile(os.path.join(REF, "wisp/csrc/external/mesh2sdf_kernel.cu")), reason="reference tree absent")
def test_oracle_directions_and_threshold_are_the_reference_kernels():
    src = open(os.path.join(REF, "wisp/csrc/external/mesh2sdf_kernel.cu")).read()
    quad = src[src.index("void kernel_mesh2sdf_quad("):]                  # the kernel mesh_to_sdf_cuda launches (:334)
    table = quad[quad.index("stab_dir_table[13][3]"):]
    table = table[:table.index(";")]
    rows = re.findall(r"\{\s*([-0-9.f]+)\s*,\s*([-0-9.f]+)\s*,\s*([-0-9.f]+)\s*\}", table)
    got = np.array([[float(np.float32(float(x.rstrip("f")))) for x in r] for r in rows])
    assert got.shape == (13, 3) and np.array_equal(got, oracle.DIRS)
    assert "det > -1e-8 && det < 1e-8" in quad[:quad.index("kernel_quad_aggr")] and oracle.DET_EPS == 1e-8


@pytest.mark.skipif(not os.path.isfile(os.path.join(REF, "wisp/ops/spc/sampling.py")), reason="reference tree absent")
def test_sample_spc_matches_reference_draws():
    from wisp.ops.spc import sample_spc
    ref, = _exec_reference("wisp/ops/spc/sampling.py", ["sample_spc"])
    corners = torch.randint(0, 32, (50, 3), dtype=torch.int16)
    torch.manual_seed(7)
    want = ref(corners, 5, 6)
    torch.manual_seed(7)
    got = sample_spc(corners, 5, 6)
    assert got.shape == (300, 3) and torch.equal(got, want)


def test_sample_spc_stays_inside_its_voxels():
    from wisp.ops.spc import sample_spc
    corners = torch.tensor([[0, 0, 0], [3, 1, 2]], dtype=torch.int16)
    s = sample_spc(corners, 2, 100).reshape(2, 100, 3)
    cell = torch.floor((s + 1) / 2 * 4)
    assert torch.equal(cell, corners[:, None, :].float().expand_as(cell))


def test_sdf_datasets_validate_without_a_device(tmp_path):
    from wisp.accelstructs import OctreeAS
    from wisp.datasets import MeshSampledSDFDataset, OctreeSampledSDFDataset
    dense = OctreeAS.make_dense(2)
    assert not OctreeSampledSDFDataset.supports_blas(dense)
    pc = OctreeAS.from_pointcloud(torch.rand(100, 3) * 2 - 1, 3) if not torch.cuda.is_available() else dense
    assert not OctreeSampledSDFDataset.supports_blas(pc)
    with pytest.raises(RuntimeError, match="not initialized from a mesh"):
        OctreeSampledSDFDataset(dense, split='train')
    with pytest.raises(FileNotFoundError, match="does not exist"):
        MeshSampledSDFDataset(str(tmp_path / "missing.obj"), split='train')
    ply = tmp_path / "mesh.ply"
    ply.write_text("ply\n")
    with pytest.raises(FileNotFoundError, match="does not support the mesh format"):
        MeshSampledSDFDataset(str(ply), split='train')
    obj = oracle.write_obj(tmp_path / "tri.obj", *oracle.single_triangle())
    with pytest.raises(NotImplementedError):
        MeshSampledSDFDataset(obj, split='train', sample_tex=True)
    fake = OctreeAS.make_dense(2)
    fake.extent['vertices'], fake.extent['faces'] = torch.zeros(3, 3), torch.zeros(1, 3, dtype=torch.long)
    assert OctreeSampledSDFDataset.supports_blas(fake)
    with pytest.raises(NotImplementedError):
        OctreeSampledSDFDataset(fake, split='train', sample_tex=True)


def test_sdf_dataset_constructor_schemas_match_reference_api():
    from wisp.datasets import MeshSampledSDFDataset, OctreeSampledSDFDataset, SDFDataset
    sig = inspect.signature(MeshSampledSDFDataset.__init__)
    assert [(k, v.default) for k, v in list(sig.parameters.items())[1:]] == [
        ('mesh_path', inspect.Parameter.empty), ('split', inspect.Parameter.empty), ('transform', None), ('sample_mode', None),
        ('num_samples', 100000), ('get_normals', False), ('sample_tex', False), ('mode_norm', 'sphere')]
    sig = inspect.signature(OctreeSampledSDFDataset.__init__)
    assert [(k, v.default) for k, v in list(sig.parameters.items())[1:]] == [
        ('occupancy_struct', inspect.Parameter.empty), ('split', inspect.Parameter.empty), ('transform', None),
        ('sample_mode', None), ('num_samples', 100000), ('sample_tex', False), ('samples_per_voxel', 32)]
    assert issubclass(MeshSampledSDFDataset, SDFDataset) and issubclass(OctreeSampledSDFDataset, SDFDataset)


@pytest.mark.skipif(not os.path.isfile(os.path.join(REF, "wisp/datasets/formats/octree_sdf_dataset.py")), reason="reference tree absent")
def test_sdf_dataset_schemas_equal_the_reference_sources():
    import ast
    from wisp.datasets import MeshSampledSDFDataset, OctreeSampledSDFDataset
    for rel, cls in (("mesh_sdf_dataset.py", MeshSampledSDFDataset), ("octree_sdf_dataset.py", OctreeSampledSDFDataset)):
        tree = ast.parse(open(os.path.join(REF, "wisp/datasets/formats", rel)).read())
        init = next(n for c in tree.body if isinstance(c, ast.ClassDef) and c.name == cls.__name__
                    for n in c.body if isinstance(n, ast.FunctionDef) and n.name == "__init__")
        names = [a.arg for a in init.args.args][1:]
        defaults = [ast.literal_eval(d) for d in init.args.defaults]
        sig = inspect.signature(cls.__init__)
        assert list(sig.parameters)[1:] == names
        assert [v.default for v in list(sig.parameters.values())[-len(defaults):]] == defaults


def test_reference_named_external_surface_and_c_abi():
    import wisp._C as C
    assert len(inspect.signature(C.external.mesh_to_sdf_cuda).parameters) == 2
    assert len(inspect.signature(C.external.mesh_to_sdf_triangle_cuda).parameters) == 2
    assert C.lib.wisp_mesh_sdf_workspace_bytes(1000, 10) >= 10 * 88 * 8 + 1000 * 12
    with pytest.raises(RuntimeError, match="GPU tensor"):
        C.external.mesh_to_sdf_cuda(torch.zeros(4, 3, dtype=torch.float64), torch.zeros(1, 3, 3, dtype=torch.float64))


@pytest.mark.skipif(not kernel_meta.available(LIB), reason="libwisp_hip.so not built or llvm-readelf missing")
def test_mesh_sdf_kernels_have_zero_scratch_and_allowed_workgroups():
    meta = kernel_meta.kernels(LIB)
    names = kernel_meta.demangled(list(meta))
    ours = {names[k]: v for k, v in meta.items() if "mesh_sdf_" in names[k]}
    assert len(ours) == 7, sorted(ours)                  # prep, 4 main (distance / triangle x scalar / LDS), 2 finalize
    for name, v in ours.items():
        assert v["scratch"] == 0 and v["wg"] in (64, 128, 256, 512, 1024), (name, v)
    for name, v in ours.items():
        if "main_kernel<true, false>" in name or "main_kernel<false, false>" in name:
            assert v["vgpr"] <= 128, (name, v)            # 4 waves per SIMD for the scalar-load form (measured: 107)
