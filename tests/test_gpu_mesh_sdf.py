"""GPU: wisp._C.external.mesh_to_sdf_cuda / mesh_to_sdf_triangle_cuda (csrc/mesh_sdf.hip) against the numpy oracle of
tests/mesh_sdf_oracle.py on procedural meshes; bitwise split invariance of the order-free combine; compute_sdf / closest_point
semantics; the mesh-sampled SDF datasets end to end on a torus OBJ, with SDFTrainer and SDFTrainStep on top."""
import numpy as np
import pytest
import torch

import mesh_sdf_oracle as oracle

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _gpu(points, V, F, with_triangle=False, **kw):
    import wisp._C as C
    P = torch.as_tensor(points, dtype=torch.float64, device=DEV)
    T = torch.as_tensor(np.asarray(V)[np.asarray(F)], dtype=torch.float64, device=DEV)
    return C.mesh_to_sdf(P, T, with_triangle=with_triangle, **kw).cpu().numpy()


def _check_parity(P, V, F, max_ambiguous=None, on_surface=False):
    P = np.asarray(P, dtype=np.float64)
    T = np.asarray(V)[np.asarray(F)]
    want, _, amb, mind = oracle.mesh_sdf(P, T)
    if max_ambiguous is not None:
        assert amb.mean() < max_ambiguous, amb.mean()
    got = _gpu(P, V, F)
    close = oracle.sdf_close(got, want)
    if on_surface:
        # points ON edges / vertices: the face-or-edge choice follows the sign of a dot product that is zero up to rounding, and
        # the edge case's float-rounded clamp parameter moves the nearest edge point by up to |e| 2^-24
        longest = np.linalg.norm(T - T[:, [1, 2, 0]], axis=-1).max()
        close |= np.abs(np.abs(got) - np.abs(want)) <= longest * 2.0 ** -23
    assert np.all(close), np.abs(np.abs(got) - np.abs(want)).max()
    assert np.array_equal((got < 0)[~amb], (want < 0)[~amb]), np.flatnonzero(((got < 0) != (want < 0)) & ~amb)[:10]
    out = _gpu(P, V, F, with_triangle=True)
    n = P.shape[0]
    assert out.shape == (2 * n,) and np.array_equal(out[:n], got)
    idx = out[n:].astype(np.int64)
    assert np.array_equal(out[n:], idx.astype(np.float64))
    ok = idx >= 0
    assert np.array_equal(ok, np.isfinite(mind))
    # tie rule: the chosen triangle's float distsq is the minimum (within the two-ulp tolerance of the float rounding)
    fd = oracle.triangle_distsq(P[ok], oracle.Prepared(T), sel=idx[ok])
    assert np.all(np.abs(fd - mind[ok]) <= 5e-7 * mind[ok] + 1e-12)
    return got, amb


MESHES = {"box": lambda: oracle.box(0.5), "icosphere": lambda: oracle.icosphere(2, 0.8), "torus": lambda: oracle.torus(),
          "degenerate": oracle.degenerate_mesh, "single": oracle.single_triangle}


@pytest.mark.parametrize("name", sorted(MESHES))
def test_parity_random_points(name):
    V, F = MESHES[name]()
    rng = np.random.default_rng(hash(name) % 1000)
    P = rng.uniform(-1.3, 1.3, (1537, 3))                  # not a multiple of the 512-point tile; some points outside [-1, 1]^3
    _check_parity(P, V, F, max_ambiguous=1e-3)


@pytest.mark.parametrize("name", ["box", "icosphere", "torus"])
def test_parity_on_vertices_edges_and_tiny_sets(name):
    V, F = MESHES[name]()
    T = V[F]
    mids = (T[:, [0, 1, 2]] + T[:, [1, 2, 0]]) / 2
    P = np.concatenate([V, mids.reshape(-1, 3)[:300], T.mean(1)[:100]])
    _check_parity(P, V, F, on_surface=True)
    _check_parity(P[:1], V, F, on_surface=True)              # N = 1
    _check_parity(P[:77], V, F, on_surface=True)


def test_parity_bumpy_sphere_80k_triangles_million_points():
    V, F = oracle.bumpy_sphere(6)
    assert F.shape[0] == 81920
    rng = np.random.default_rng(5)
    P = rng.uniform(-1.0, 1.0, (1_000_000, 3))
    got = _gpu(P, V, F)
    sub = rng.choice(P.shape[0], 256, replace=False)
    want, _, amb, _ = oracle.mesh_sdf(P[sub], V[F])
    assert amb.mean() < 1e-2
    assert np.all(oracle.sdf_close(got[sub], want))
    assert np.array_equal((got[sub] < 0)[~amb], (want < 0)[~amb])
    r = np.linalg.norm(P, axis=1)
    true_r = oracle.bumpy_radius(P / r[:, None])
    far = np.abs(r - true_r) > 0.02
    assert np.array_equal((got < 0)[far], (r < true_r)[far])


def test_split_invariance_is_bitwise():
    import wisp._C as C
    from wisp.ops.mesh import compute_sdf
    V, F = oracle.torus(nu=64, nv=32)
    rng = np.random.default_rng(9)
    P = torch.as_tensor(rng.uniform(-1.1, 1.1, (3001, 3)), device=DEV)
    T = torch.as_tensor(V[F], device=DEV)
    base = C.mesh_to_sdf(P, T, with_triangle=True)
    for ranges, cap in ((1, 0), (3, 0), (7, 0), (64, 0), (1000, 0), (0, 3001 * 37), (5, 1024 * 100)):
        got = C.mesh_to_sdf(P, T, with_triangle=True, triangle_ranges=ranges, max_pairs_per_launch=cap)
        assert torch.equal(got.view(torch.int64), base.view(torch.int64)), (ranges, cap)
    assert torch.equal(C.mesh_to_sdf(P, T, with_triangle=True).view(torch.int64), base.view(torch.int64))     # a second run
    Vt, Ft = torch.as_tensor(V), torch.as_tensor(F)
    full = compute_sdf(Vt, Ft, P)
    assert torch.equal(full[:, 0].view(torch.int64), base[:3001].view(torch.int64))
    for split in (1, 100, 1000, 2999):
        assert torch.equal(compute_sdf(Vt, Ft, P, split_size=split).view(torch.int64), full.view(torch.int64)), split


def test_compute_sdf_and_closest_point_semantics():
    from wisp.ops.mesh import closest_point, compute_sdf
    V, F = oracle.icosphere(2, 0.8)
    rng = np.random.default_rng(11)
    P = torch.from_numpy(rng.uniform(-1, 1, (700, 3))).float()                 # float32 on the host
    sdf = compute_sdf(torch.from_numpy(V).float(), torch.from_numpy(F), P)
    assert sdf.shape == (700, 1) and sdf.dtype == torch.float64 and sdf.is_cuda
    d, hit, tidx = closest_point(torch.from_numpy(V), torch.from_numpy(F), P)
    assert d.shape == (700,) and d.dtype == torch.float64 and hit.shape == (700, 3) and hit.dtype == torch.float64
    assert tidx.shape == (700,) and tidx.dtype == torch.int64 and d.is_cuda and hit.is_cuda
    assert torch.equal(compute_sdf(torch.from_numpy(V), torch.from_numpy(F), P)[:, 0], d)
    T = torch.from_numpy(V)[torch.from_numpy(F)].to(DEV)[tidx]
    Pd = P.double().to(DEV)
    # the hit point lies on its triangle (barycentrics in [0, 1] up to rounding) and |p - hit| = |dist|
    n = torch.cross(T[:, 1] - T[:, 0], T[:, 2] - T[:, 0], dim=1)
    assert float(((hit - T[:, 0]) * n).sum(1).abs().max()) < 1e-12
    for k in range(3):
        e = T[:, (k + 1) % 3] - T[:, k]
        assert float((torch.cross(e, hit - T[:, k], dim=1) * n).sum(1).min()) > -1e-12
    assert torch.allclose((Pd - hit).norm(dim=1), d.abs(), rtol=5e-7, atol=1e-8)
    with pytest.raises(RuntimeError):
        compute_sdf(torch.from_numpy(V), torch.zeros(0, 3, dtype=torch.long), P)            # F == 0
    import wisp._C as C
    with pytest.raises(RuntimeError, match="float64"):
        C.external.mesh_to_sdf_cuda(Pd.float(), torch.as_tensor(V[F], device=DEV))
    with pytest.raises(RuntimeError):
        C.external.mesh_to_sdf_cuda(Pd[:, :2].contiguous(), torch.as_tensor(V[F], device=DEV))


@pytest.fixture(scope="module")
def torus_obj(tmp_path_factory):
    return oracle.write_obj(tmp_path_factory.mktemp("mesh") / "torus.obj", *oracle.torus(nu=96, nv=48))


def _torus_sdf_after_normalisation(P):
    # load_obj + normalize('sphere'): the torus is centred already; its farthest vertex (R + r = 0.85) goes to 1
    s = 1.0 / 0.85
    return oracle.torus_sdf(P / s, R=0.6, r=0.25) * s


FACETING = 0.02      # 96 x 48 grid: the chordal error of the tube and the ring, after scaling by 1 / 0.85, is below 0.01


def test_octree_sampled_dataset_on_a_torus(torus_obj):
    from wisp.accelstructs import OctreeAS
    from wisp.datasets import OctreeSampledSDFDataset, SDFBatch
    torch.manual_seed(0)
    blas = OctreeAS.from_mesh(torus_obj, level=6, num_samples_on_mesh=1_000_000)
    assert OctreeSampledSDFDataset.supports_blas(blas)
    ds = OctreeSampledSDFDataset(blas, split='train', samples_per_voxel=4, num_samples=20000)
    cells = int(blas.pyramid[0, 6])
    per_mode = cells * 4
    pool = ds.data_pool
    assert pool['coords'].is_cuda and pool['sdf'].dtype == torch.float64 and pool['sdf'].shape == (ds.pool_size, 1)
    # default modes ['rand', 'near', 'near', 'trace', 'trace']: 5 * cells * 4 samples, minus the 'near' ones outside [-1, 1]^3
    assert 3 * per_mode <= ds.pool_size <= 5 * per_mode
    assert float(pool['coords'].abs().max()) <= 1.0
    want = _torus_sdf_after_normalisation(pool['coords'].double().cpu().numpy())
    assert np.all(np.abs(pool['sdf'][:, 0].cpu().numpy() - want) <= FACETING)
    trace = pool['sdf'][-2 * per_mode:]
    assert float(trace.abs().max()) <= FACETING
    assert len(ds) == 20000 and ds.coordinates.shape == (20000, 3)
    ds.resample()
    b = ds.get_batch(torch.arange(10, device=DEV))
    assert isinstance(b, SDFBatch) and b['coords'].shape == (10, 3) and b['sdf'].shape == (10, 1)
    rows = {tuple(r) for r in pool['coords'].cpu().numpy().tolist()}
    assert all(tuple(r) in rows for r in ds.data['coords'][:200].cpu().numpy().tolist())


@pytest.mark.parametrize("normals", [False, True])
def test_mesh_sampled_dataset_on_a_torus(torus_obj, normals):
    from wisp.datasets import MeshSampledSDFDataset
    torch.manual_seed(1)
    ds = MeshSampledSDFDataset(torus_obj, split='train', num_samples=4000, get_normals=normals)
    assert len(ds) == 20000 and ds.data['coords'].is_cuda and ds.data['sdf'].shape == (20000, 1)
    want = _torus_sdf_after_normalisation(ds.data['coords'].double().cpu().numpy())
    assert np.all(np.abs(ds.data['sdf'][:, 0].cpu().numpy() - want) <= FACETING)
    if normals:
        assert ds.data['normals'].shape == (20000, 3) and float(ds.data['sdf'].abs().max()) <= FACETING
    else:
        assert 'normals' not in ds.data
    before = ds.data['coords'].clone()
    ds.resample()
    assert ds.data['coords'].shape == before.shape and not torch.equal(ds.data['coords'], before)


def test_sdf_training_runs_on_the_mesh_datasets(torus_obj):
    from wisp.accelstructs import OctreeAS
    from wisp.datasets import MeshSampledSDFDataset, OctreeSampledSDFDataset
    from wisp.models import Pipeline
    from wisp.models.grids import OctreeGrid
    from wisp.models.nefs import NeuralSDF
    from wisp.trainers import SDFTrainer, SDFTrainStep, ConfigSDFTrainer, ConfigAdam, ConfigDataloader
    torch.manual_seed(2)
    blas = OctreeAS.from_mesh(torus_obj, level=5, num_samples_on_mesh=1_000_000)
    ods = OctreeSampledSDFDataset(blas, split='train', samples_per_voxel=8, num_samples=30000)
    mds = MeshSampledSDFDataset(torus_obj, split='train', num_samples=3000)

    def make():
        grid = OctreeGrid(blas, feature_dim=16, num_lods=3, multiscale_type='sum', feature_std=0.05)
        return NeuralSDF(grid, pos_embedder='none', position_input=True, hidden_dim=128, num_layers=1).to(DEV)

    step = SDFTrainStep(make(), lr=1e-3, eps=1e-15)
    losses = []
    for i in range(300):
        b = ods.get_batch(torch.randint(0, len(ods), (512,), device=DEV))
        losses.append(float(step.step(b['coords'].float().contiguous(), b['sdf'].float().contiguous())))
    first, last = np.mean(losses[:10]), np.mean(losses[-10:])
    print(f"SDFTrainStep on OctreeSampledSDFDataset: mean loss of the first / last 10 steps {first:.4g} / {last:.4g}")
    assert np.isfinite(losses).all() and last < 0.5 * first, (first, last)
    cfg = ConfigSDFTrainer(optimizer=ConfigAdam(lr=1e-3, eps=1e-15), dataloader=ConfigDataloader(batch_size=512), max_epochs=2,
                           resample=True)
    tr = SDFTrainer(cfg, Pipeline(make(), None), mds, device=DEV)
    coords_before = mds.data['coords'].clone()
    tr.is_optimization_running = True
    for _ in range(tr.iterations_per_epoch + 1):
        tr.iterate()
    assert tr.epoch >= 1 and np.isfinite(tr.tracker.metrics.total_loss)
    assert not torch.equal(mds.data['coords'], coords_before)          # post_epoch resampled the dataset
