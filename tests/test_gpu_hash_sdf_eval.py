"""GPU: the fused evaluation of a hash-grid SDF field (csrc/hash_sdf_eval.hip) - query with its IoU counters, central-difference
gradient and the fused marching iteration - against the float64 reference of tests/hash_sdf_eval_ref.py: bit for bit on exactly
representable inputs, against the modular path's own error on generic ones, bit for bit against the two-launch marching loop - and
what is built on them: PackedSDFTracer, wisp.ops.sdf, SDFTrainer.validate, OfflineRenderer, scripts/train_nglod.py --grid hash.
Every measured margin is appended to profiles/hash_sdf_eval_test_margins.jsonl when WISP_HASH_SDF_EVAL_MARGINS names a file."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import hash_sdf_eval_ref as R
from gpu_helpers import STATE, make_rays, march_start, shell_blas

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
NS = (1, 15, 17, 1000)
F32, F16, BF16 = torch.float32, torch.float16, torch.bfloat16


def record(name, **values):
    path = os.environ.get("WISP_HASH_SDF_EVAL_MARGINS")
    if path:
        with open(path, "a") as f:
            f.write(json.dumps(dict(name=name, **{k: (float(v) if not isinstance(v, (int, str)) else v) for k, v in values.items()})) + "\n")


def dev_field(fld):
    """the kernels' field dict (kind 'hash') from a reference field, no nef in between"""
    return dict(kind='hash', codebook=fld["table"].to(DEV).contiguous(), begin_idxes=[int(b) for b in fld["begin"]],
                resolutions=list(fld["resolutions"]), feature_dim=int(fld["table"].shape[1]), codebook_bitwidth=fld["bitwidth"],
                multiscale=fld["multiscale"], zero_from_col=R.zero_from_col(fld), w1=fld["w1"].to(DEV).contiguous(),
                b1=fld["b1"].to(DEV).contiguous(), w2=fld["w2"].to(DEV).contiguous(), b2=fld["b2"].to(DEV).contiguous())


def nef_of(fld, blas=None):
    """NeuralSDF over a HashGrid carrying a reference field's parameters"""
    from wisp.models.grids import HashGrid
    from wisp.models.nefs import NeuralSDF
    F = int(fld["table"].shape[1])
    grid = HashGrid.from_resolutions(blas, feature_dim=F, resolutions=list(fld["resolutions"]), multiscale_type=fld["multiscale"],
                                     feature_std=0.01, codebook_bitwidth=fld["bitwidth"])
    nef = NeuralSDF(grid, pos_embedder='none', position_input=True, hidden_dim=fld["w1"].shape[0], num_layers=1)
    with torch.no_grad():
        assert grid.codebook.feats.shape == fld["table"].shape
        grid.codebook.feats.data = fld["table"].clone()
        nef.decoder.layers[0].weight.copy_(fld["w1"]); nef.decoder.layers[0].bias.copy_(fld["b1"])
        nef.decoder.lout.weight.copy_(fld["w2"].reshape(1, -1)); nef.decoder.lout.bias.copy_(fld["b2"])
    return nef.to(DEV).eval()


_cache = {}

# pairwise cover of hidden 1 / 17 / 128 / 256, F 2 / 4 / 8, 'cat' / 'sum', lod_idx 0 / middle / last, f32 / f16 / bf16 tables
EXACT = [(1, 8, 'cat', 3, F32), (17, 4, 'cat', 0, F16), (128, 2, 'cat', 2, BF16), (256, 8, 'sum', 3, F32), (128, 4, 'sum', 1, F16),
         (17, 2, 'sum', 3, BF16), (256, 4, 'cat', 3, BF16), (1, 2, 'sum', 2, F32), (128, 8, 'cat', 2, F16), (17, 8, 'cat', 1, BF16),
         (256, 2, 'cat', 1, F16), (1, 4, 'sum', 0, BF16), (128, 8, 'cat', 0, F32), (256, 4, 'cat', 0, F32), (1, 8, 'sum', 2, F16),
         (17, 8, 'sum', 0, F32), (17, 2, 'cat', 0, F32)]


def exact(kind, hidden, F, multiscale, lod_idx, dtype):
    """one 1000-point exact case per key, its float64 reference computed once"""
    key = (kind, hidden, F, multiscale, lod_idx, dtype)
    if key not in _cache:
        if kind == "query":
            case = R.exact_case(hidden, F, multiscale, lod_idx, n=1000, seed=5, dtype=dtype)
            case["want"] = R.reference(case["field"], case["coords"])
        else:
            case = R.exact_gradient_case(hidden, F, multiscale, lod_idx, n=1000, seed=6, dtype=dtype)
            case["want"] = R.gradient_reference(case["field"], case["coords"], case["eps"])
            pos = R.offsets(case["coords"], case["eps"]).reshape(-1, 3)
            case["six"], case["want_six"] = pos, R.reference(case["field"], pos)
        case["dev"] = dev_field(case["field"])
        _cache[key] = case
    return _cache[key]


# ------------------------------------------------------------------------------------------------ 1. exact inputs
@pytest.mark.parametrize("hidden,F,multiscale,lod_idx,dtype", EXACT)
def test_query_equals_float64_bit_for_bit_on_exact_inputs(hidden, F, multiscale, lod_idx, dtype):
    import wisp._C as C
    case = exact("query", hidden, F, multiscale, lod_idx, dtype)
    for n in NS:
        got = C.sdf_query(case["coords"][:n].to(DEV), case["dev"])
        assert got.shape == (n, 1)
        assert torch.equal(got.double().cpu(), case["want"][:n]), (hidden, F, multiscale, lod_idx, dtype, n)
    assert len(torch.unique(case["want"])) > 20                         # (no dead decoder among the cases)


@pytest.mark.parametrize("hidden,F,multiscale,lod_idx,dtype", EXACT)
def test_gradient_equals_float64_bit_for_bit_on_exact_inputs(hidden, F, multiscale, lod_idx, dtype):
    """a dyadic eps: the six positions are exact points, f+ - f- and the division by 2 eps are exact.  The six values themselves
    are checked through the query at the six positions (the gradient kernel evaluates them with the same device function)."""
    import wisp._C as C
    case = exact("gradient", hidden, F, multiscale, lod_idx, dtype)
    six = C.sdf_query(case["six"].to(DEV), case["dev"])
    assert torch.equal(six.double().cpu(), case["want_six"])
    for n in NS:
        got = C.sdf_fd_gradient(case["coords"][:n].to(DEV), case["dev"], eps=case["eps"])
        assert got.shape == (n, 3)
        assert torch.equal(got.double().cpu(), case["want"][:n]), (hidden, F, multiscale, lod_idx, dtype, n)
    assert int((case["want"] != 0).sum()) > 100


def test_empty_batch_and_python_argument_checks():
    import wisp._C as C
    case = exact("query", 17, 4, 'cat', 0, F16)
    assert C.sdf_query(torch.zeros(0, 3, device=DEV), case["dev"]).shape == (0, 1)
    assert C.sdf_fd_gradient(torch.zeros(0, 3, device=DEV), case["dev"]).shape == (0, 3)
    with pytest.raises(RuntimeError, match="GPU tensor"):
        C.sdf_query(torch.zeros(4, 3), case["dev"])
    with pytest.raises(RuntimeError, match="32 feature columns"):
        C.sdf_query(torch.zeros(4, 3, device=DEV), dict(case["dev"], resolutions=[4, 8, 16, 32] * 3, feature_dim=4,
                                                        begin_idxes=[0] * 12 + [case["dev"]["codebook"].shape[0]],
                                                        w1=torch.zeros(17, 51, device=DEV)))


# ------------------------------------------------------------------------------------------------ 2. generic inputs
GENERIC = [(0, 128, 8, 'cat', 3, F32), (1, 128, 8, 'cat', 3, F32), (0, 17, 4, 'cat', 2, F32), (1, 256, 8, 'sum', 3, F32),
           (0, 128, 2, 'sum', 1, F32), (1, 128, 8, 'cat', 2, F16), (0, 128, 4, 'sum', 3, BF16), (1, 1, 8, 'cat', 0, F32)]


def generic_setup(res, hidden, F, multiscale, lod_idx, dtype, n=1000):
    key = ("generic", res, hidden, F, multiscale, lod_idx, dtype)
    if key not in _cache:
        fld = R.generic_field(R.GENERIC_RES[res], hidden, F=F, multiscale=multiscale, lod_idx=lod_idx, seed=3 + res, dtype=dtype)
        coords = R.generic_points(n, seed=9)
        _cache[key] = (fld, nef_of(fld), coords, coords.to(DEV), R.reference(fld, coords))
    return _cache[key]


@pytest.mark.parametrize("res,hidden,F,multiscale,lod_idx,dtype", GENERIC)
def test_query_error_is_within_twice_the_modular_paths(res, hidden, F, multiscale, lod_idx, dtype):
    """fused and modular path differ by the summation order of the decoder only: the fused error against float64 (same tensors)
    is at most twice the modular path's own - points inside the cube, on c = +-1 and outside it (clamped)"""
    from wisp.ops.sdf import fused_sdf_field
    import wisp._C as C
    fld, nef, coords, cd, want = generic_setup(res, hidden, F, multiscale, lod_idx, dtype)
    fused = fused_sdf_field(nef, lod_idx)
    assert fused is not None and fused["kind"] == "hash" and fused["zero_from_col"] == R.zero_from_col(fld)
    got = C.sdf_query(cd, fused).double().cpu()
    with torch.no_grad():
        mod = nef(coords=cd, lod_idx=lod_idx, channels="sdf").double().cpu()
    for name, pick in (("inside", (coords.abs() < 1).all(1)), ("face", (coords.abs() == 1).any(1) & (coords.abs() <= 1).all(1)),
                       ("outside", (coords.abs() > 1).any(1))):
        assert int(pick.sum()) > 100, name
        e_fused, e_mod = float((got - want)[pick].abs().max()), float((mod - want)[pick].abs().max())
        record("query_generic", res=str(R.GENERIC_RES[res]), hidden=hidden, F=F, multiscale=multiscale, lod_idx=lod_idx, dtype=str(dtype),
               where=name, err_fused=e_fused, err_modular=e_mod, fused_vs_modular=float((got - mod)[pick].abs().max()))
        print(f"{R.GENERIC_RES[res]} h{hidden} F{F} {multiscale} lod{lod_idx} {dtype} {name}: fused {e_fused:.3e} modular {e_mod:.3e}")
        assert e_fused <= 2.0 * e_mod, (name, e_fused, e_mod)


def ulps32(a, b):
    """distance of fp32 tensor a from float64 tensor b in units of the fp32 spacing at |b|"""
    spacing = torch.from_numpy(np.spacing(np.abs(b.numpy()).astype(np.float32)).astype(np.float64))
    return (a.double() - b).abs() / spacing


GRAD_MARGIN = 4.0


@pytest.mark.parametrize("res,hidden,F,multiscale,lod_idx,dtype", [GENERIC[1], GENERIC[2], GENERIC[3], GENERIC[5]])
def test_gradient_is_the_central_difference_of_the_querys_own_values(res, hidden, F, multiscale, lod_idx, dtype):
    """each component within 4 fp32 ulps of (f+ - f-) / 0.01 evaluated in float64 from wisp_hash_sdf_query's values at
    x +- 0.005f - with the subtraction taken in float64, and with it taken in fp32 as the kernel takes it"""
    from wisp.ops.sdf import fused_sdf_field, sdf_fd_gradient
    import wisp._C as C
    fld, nef, coords, cd, _ = generic_setup(res, hidden, F, multiscale, lod_idx, dtype)
    fused = fused_sdf_field(nef, lod_idx)
    six = C.sdf_query(R.offsets(coords, 0.005).reshape(-1, 3).to(DEV), fused)[:, -1].cpu().reshape(3, 2, -1)
    diff32 = six[:, 0] - six[:, 1]                                       # the kernel's fp32 subtraction
    want = (diff32.double() / 0.01).T
    want_f64 = ((six[:, 0].double() - six[:, 1].double()) / 0.01).T
    for n in NS:
        got = sdf_fd_gradient(nef, cd[:n], lod_idx).cpu()
        u, u64 = ulps32(got, want[:n]), ulps32(got, want_f64[:n])
        record("gradient_generic", res=str(R.GENERIC_RES[res]), hidden=hidden, multiscale=multiscale, lod_idx=lod_idx, dtype=str(dtype), n=n,
               max_ulps=float(u.max()), max_ulps_vs_f64_difference=float(u64.max()))
        assert float(u.max()) <= GRAD_MARGIN, (n, float(u.max()))
        assert float(u64.max()) <= GRAD_MARGIN, (n, float(u64.max()))
    assert float(want.abs().max()) > 1e-3


# ------------------------------------------------------------------------------------------------ 3. IoU counters
@pytest.mark.parametrize("res,hidden,F,multiscale,lod_idx,dtype", [GENERIC[1], GENERIC[3]])
def test_iou_counts(res, hidden, F, multiscale, lod_idx, dtype):
    from wisp.ops.sdf import compute_sdf_iou
    import wisp._C as C
    fld, nef, coords, cd, want = generic_setup(res, hidden, F, multiscale, lod_idx, dtype)
    moved = dict(fld, b2=fld["b2"] - float(want.median()))               # move the output bias so that both signs occur
    dev = dev_field(moved)
    gts = R.sphere_sdf(coords).to(DEV)
    runs = []
    for _ in range(3):
        counts = torch.zeros(2, dtype=torch.int64, device=DEV)
        out = C.sdf_query(cd, dev, gts=gts, counts=counts)
        runs.append(counts.cpu().tolist())
    pred = out[:, 0]
    same_launch = [int(((pred < 0) & (gts < 0)).sum()), int(((pred < 0) | (gts < 0)).sum())]
    assert runs[0] == same_launch and runs[1] == runs[0] and runs[2] == runs[0]             # the launch's own output; reruns
    only = torch.zeros(2, dtype=torch.int64, device=DEV)
    assert C.sdf_query(cd, dev, gts=gts, counts=only, with_out=False) is None and only.cpu().tolist() == runs[0]   # out = NULL
    assert 0 < runs[0][0] < runs[0][1] < coords.shape[0]
    assert 100.0 * (runs[0][0] / runs[0][1]) == compute_sdf_iou(pred[:, None], gts[:, None])
    C.sdf_query(cd[:17], dev, gts=gts[:17], counts=only, with_out=False)                    # a second launch adds
    extra = [int(((pred[:17] < 0) & (gts[:17] < 0)).sum()), int(((pred[:17] < 0) | (gts[:17] < 0)).sum())]
    assert only.cpu().tolist() == [runs[0][0] + extra[0], runs[0][1] + extra[1]]
    record("iou_counts", res=str(R.GENERIC_RES[res]), multiscale=multiscale, n=coords.shape[0], inter=runs[0][0], union=runs[0][1])


# ------------------------------------------------------------------------------------------------ 4. one marching iteration
@pytest.mark.parametrize("multiscale,dtype", [('cat', F32), ('sum', F16)])
def test_fused_marching_iteration_equals_step_then_query_bit_for_bit(multiscale, dtype):
    """wisp_hash_sdf_trace_step_fused against wisp_sphere_trace_step followed by wisp_hash_sdf_query at x of the active packs
    times scale, from a real raytrace of 300 rays through a level-4 shell: every state array bitwise equal after one iteration
    and after 24 - both sides run the same statements"""
    import copy
    import wisp._C as C
    _, blas = shell_blas(4, 0.625, 0.18)
    fld = R.generic_field(R.GENERIC_RES[0], 128, F=8 if multiscale == 'cat' else 4, multiscale=multiscale, lod_idx=3, seed=21, dtype=dtype)
    nef = nef_of(fld, blas)
    rays, rt, depth, st0 = march_start(nef, 300, 151)
    P = st0.t.shape[0]
    assert 100 < P <= 300
    with torch.no_grad():                                                # distances of about a cell's size, mostly positive
        v = C.sdf_query(st0.x, dev_field(fld))
    fld = dict(fld, b2=fld["b2"] - float(v.median()) + 0.15)
    dev = dev_field(fld)
    scale, min_dis, dist_max = 0.8, 0.0003, float(rays.dist_max)
    a, b = copy.deepcopy(st0), copy.deepcopy(st0)
    counter = torch.zeros(1, dtype=torch.int32, device=DEV)

    def fused(st, first, cnt=None):
        C.sdf_trace_step_field(first, st.o, st.d, depth, rt.pidx, dist_max, min_dis, min_dis * 5, st.t, st.dist, st.dist_prev,
                               st.active, st.hit, st.nug, st.nug_next, st.cell, st.x, dev, scale, cnt)

    def query(st):
        sel = st.active.bool()
        if bool(sel.any()):
            st.dist[sel] = (C.sdf_query(st.x[sel], dev) * scale).reshape(-1)

    def same(where):
        for name in STATE:
            assert torch.equal(getattr(a, name), getattr(b, name)), (where, name)
    fused(a, True)
    query(b)
    same("start")
    a.dist_prev.copy_(a.dist)
    b.dist_prev.copy_(b.dist)
    for it in range(24):
        counter.zero_()
        fused(a, False, counter)
        a.nug, a.nug_next = a.nug_next, a.nug
        C.sphere_trace_step(b.o, b.d, depth, rt.pidx, dist_max, min_dis, min_dis * 5, b.t, b.dist, b.dist_prev, b.active, b.hit,
                            b.nug, b.nug_next, b.cell, b.x)
        b.nug, b.nug_next = b.nug_next, b.nug
        query(b)
        same(f"iteration {it}")
        assert int(counter.item()) == int(b.active.sum())
        if it == 0:
            assert int(b.active.sum()) > 50 and not torch.equal(b.t, st0.t)
    moved = int((b.nug != st0.nug).sum())
    record("march_exact", multiscale=multiscale, dtype=str(dtype), packs=P, active_after_24=int(b.active.sum()), hits=int(b.hit.sum()),
           moved_cells=moved)
    assert int(b.active.sum()) < P and moved > 10                          # packs left or converged, and cells were jumped


# ------------------------------------------------------------------------------------------------ 5. whole tracer
# The fit.  Tables of 2^12 rows at resolutions 80 and 406 hold hundreds to thousands of cells of the shell per row, so what the table
# learning rate builds there is noise on top of the decoder's fit of the position: at grid_lr_weight 10 (the octree test's value) the
# field came out rough - the surface 0.036 .. 0.041 off the sphere, and single rays of the fused and the modular march settling on
# different wrinkles (depth apart by 3e-3 .. 1.6e-2, hit masks equal).  At grid_lr_weight 0.1 and 400 steps the same bounds hold with
# the values recorded in profiles/hash_sdf_eval_test_margins.jsonl (name "tracer"); the modular loop reruns bit for bit either way.
FIT = dict(level=5, radius=0.55, steps=400, lr=3e-3, grid_lr_weight=0.1)


def fitted_pipeline():
    """NeuralSDF over a HashGrid ('cat', 4 levels x 8 features, resolutions 16 .. 2048, tables of 2^12 rows) on the level-5 cells
    around the sphere of radius 0.55, fitted to it with SDFTrainStep (its modular launches), with a tracer"""
    from wisp.models import Pipeline
    from wisp.models.grids import HashGrid
    from wisp.models.nefs import NeuralSDF
    from wisp.tracers import PackedSDFTracer
    from wisp.trainers import SDFTrainStep
    if "fitted" not in _cache:
        cells_np, blas = shell_blas(FIT["level"], FIT["radius"], 0.15)
        torch.manual_seed(11)
        grid = HashGrid.from_geometric(blas, feature_dim=8, num_lods=4, multiscale_type='cat', feature_std=0.01, codebook_bitwidth=12,
                                       min_grid_res=16, max_grid_res=2048)
        nef = NeuralSDF(grid, pos_embedder='none', position_input=True, hidden_dim=128, num_layers=1).to(DEV)
        step = SDFTrainStep(nef, lr=FIT["lr"], grid_lr_weight=FIT["grid_lr_weight"])
        g = torch.Generator(device=DEV).manual_seed(12)
        cells = torch.from_numpy(cells_np.astype(np.float32)).to(DEV)
        for _ in range(FIT["steps"]):
            pick = torch.randint(0, cells.shape[0], (2048,), device=DEV, generator=g)
            xs = (cells[pick] + torch.rand(2048, 3, device=DEV, generator=g)) / 16 - 1
            step.step(xs, xs.norm(dim=-1, keepdim=True) - FIT["radius"])
        nef.eval()
        _cache["fitted"] = Pipeline(nef, PackedSDFTracer(num_steps=40, step_size=0.8, min_dis=0.0003))
    return _cache["fitted"]


def test_tracer_fused_iteration_equals_modular_marching(monkeypatch):
    """the bounds of test_sdf_tracer_fused_iteration_equals_modular_marching on a hash-grid field fitted to a sphere (FIT: 400
    steps of 2048 points at lr 3e-3, grid_lr_weight 0.1 - see there why): hit masks differ on at most max(2, 0.2 %) of 3000 rays, depth and xyz
    agree within 6e-4 (= 2 min_dis), the median depth difference is at most 1e-6, more than 500 hits, the surface is the sphere"""
    from wisp.core import Rays
    from wisp.tracers import PackedSDFTracer
    pipe = fitted_pipeline()
    nef, tracer = pipe.nef, pipe.tracer
    o, d = make_rays(3000, 151, radius=2.5, spread=0.7)
    rays = Rays(torch.from_numpy(o).to(DEV), torch.from_numpy(d).to(DEV), dist_min=0.0, dist_max=6.0)
    outs = []
    for fused in ("1", "0"):
        monkeypatch.setenv("WISP_SDF_FUSED", fused)
        assert (PackedSDFTracer._fused_field(nef, 3) is not None) == (fused == "1")
        outs.append(tracer(nef, rays=rays, channels=["depth", "hit"], lod_idx=3))
    a, b = outs
    hits_a, hits_b = a.hit.reshape(-1), b.hit.reshape(-1)
    differ = int((hits_a != hits_b).sum())
    both = hits_a & hits_b
    dd = (a.depth.reshape(-1)[both] - b.depth.reshape(-1)[both]).abs()
    dx = float((a.xyz[both] - b.xyz[both]).abs().max())
    off = float((b.xyz[both].norm(dim=-1) - FIT["radius"]).abs().mean())
    record("tracer", rays=3000, hits_fused=int(hits_a.sum()), hits_modular=int(hits_b.sum()), hit_masks_differ=differ,
           depth_max=float(dd.max()), depth_median=float(dd.median()), xyz_max=dx, surface_mean_abs=off)
    print(f"hits {int(hits_a.sum())} / {int(hits_b.sum())} differ {differ} depth max {float(dd.max()):.3e} median {float(dd.median()):.3e} "
          f"xyz {dx:.3e} surface {off:.4f}")
    assert int(hits_b.sum()) > 500
    assert differ <= max(2, int(0.002 * hits_b.numel())), differ
    assert float(dd.max()) <= 6e-4 and float(dd.median()) <= 1e-6
    assert dx <= 6e-4
    assert off < 0.02


# ------------------------------------------------------------------------------------------------ 6. the public surface
def test_sdf_query_and_gradient_dispatch_and_fall_back_exactly(monkeypatch):
    from wisp.ops.differential import finitediff_gradient
    from wisp.ops.sdf import fused_sdf_field, sdf_query, sdf_fd_gradient
    import wisp._C as C
    pipe = fitted_pipeline()
    nef = pipe.nef
    cd = R.generic_points(300, seed=2).to(DEV)
    gts = R.sphere_sdf(cd.cpu(), FIT["radius"]).to(DEV)
    for lod in (0, 2, 3, None):
        fld = fused_sdf_field(nef, lod)
        assert fld is not None and fld["zero_from_col"] == (3 if lod is None else lod) * 8
        assert torch.equal(sdf_query(nef, cd, lod), C.sdf_query(cd, fld))
        assert torch.equal(sdf_fd_gradient(nef, cd, lod), C.sdf_fd_gradient(cd, fld, 0.005))
    counts = torch.zeros(2, dtype=torch.int64, device=DEV)
    pred = sdf_query(nef, cd, 3, gts=gts, counts=counts)
    assert counts.cpu().tolist() == [int(((pred[:, 0] < 0) & (gts < 0)).sum()), int(((pred[:, 0] < 0) | (gts < 0)).sum())]
    with torch.no_grad():
        diff = float((pred - nef(coords=cd, lod_idx=3, channels="sdf")).abs().max())
    record("public_query", fused_vs_modular=diff)
    assert diff <= 1e-5
    monkeypatch.setenv("WISP_SDF_FUSED", "0")
    assert fused_sdf_field(nef, 3) is None
    counts.zero_()
    with torch.no_grad():
        pred = sdf_query(nef, cd, 3, gts=gts, counts=counts)
        assert torch.equal(pred, nef(coords=cd, lod_idx=3, channels="sdf"))
        assert torch.equal(sdf_fd_gradient(nef, cd, 3), finitediff_gradient(cd, lambda x: nef(coords=x, lod_idx=3, channels="sdf")))
    assert counts.cpu().tolist() == [int(((pred[:, 0] < 0) & (gts < 0)).sum()), int(((pred[:, 0] < 0) | (gts < 0)).sum())]


class _SphereSet:
    """stand-in for a mesh dataset: points around the sphere with their distances, served in batches by get_batch"""

    def __init__(self, n, seed):
        g = torch.Generator().manual_seed(seed)
        d = torch.nn.functional.normalize(torch.randn(n, 3, generator=g), dim=1)
        self.coords = (d * (FIT["radius"] + 0.1 * torch.randn(n, 1, generator=g))).to(DEV)
        self.sdf = self.coords.norm(dim=1, keepdim=True) - FIT["radius"]
        self.device = torch.device(DEV)

    def __len__(self):
        return self.coords.shape[0]

    def get_batch(self, idx):
        return dict(coords=self.coords[idx], sdf=self.sdf[idx])


class _FixedLoader:
    def __init__(self, batches):
        self.batches = batches

    def __len__(self):
        return len(self.batches)

    def __iter__(self):
        return iter(self.batches)


VALIDATE_SEED = 21


@pytest.mark.parametrize("only_last", [True, False])
def test_validate_fused_equals_modular(only_last, monkeypatch):
    """SDFTrainer.validate() through one launch per batch and LOD against WISP_SDF_FUSED=0 over the same batches: the counters
    are integers, so the scores are EQUAL unless a prediction sits within the fused-vs-modular difference of 0 - the data seed is
    one for which none does, which is asserted per batch and LOD"""
    from wisp.ops.sdf import sdf_query
    from wisp.trainers import ConfigAdam, ConfigDataloader, ConfigSDFTrainer, SDFTrainer
    pipe = fitted_pipeline()
    nef = pipe.nef
    ds = _SphereSet(1000, VALIDATE_SEED)
    monkeypatch.setattr(SDFTrainer, "_validation_metric_name", lambda self: "volumetric_iou")
    cfg = ConfigSDFTrainer(optimizer=ConfigAdam(lr=1e-3, eps=1e-15), dataloader=ConfigDataloader(batch_size=300), max_epochs=1,
                           only_last=only_last, profile_nvtx=False)
    trainer = SDFTrainer(cfg, pipe, ds, device=DEV)
    torch.manual_seed(77)
    batches = list(trainer.train_data_loader)                 # one seeded pass, then the same batches for both runs
    assert [b["coords"].shape[0] for b in batches] == [300, 300, 300, 100]
    trainer.train_data_loader = _FixedLoader(batches)
    loss_lods = [3] if only_last else [0, 1, 2, 3]
    for bi, b in enumerate(batches):
        for lod in loss_lods:
            with torch.no_grad():
                pm = nef(coords=b["coords"], lod_idx=lod, channels="sdf").reshape(-1)
            pf = sdf_query(nef, b["coords"], lod).reshape(-1)
            diff = float((pf - pm).abs().max())
            near = int((pm.abs() <= diff).sum())
            record("validate", only_last=int(only_last), batch=bi, lod=lod, fused_vs_modular=diff, min_abs_pred=float(pm.abs().min()), near=near)
            assert near == 0, (bi, lod, diff, float(pm.abs().min()))

    def run():
        calls = []
        monkeypatch.setattr(trainer.tracker, "log_metric", lambda *a, **k: calls.append(a), raising=False)
        return trainer.validate()["volumetric_iou"], calls
    fused_means, fused_calls = run()
    monkeypatch.setenv("WISP_SDF_FUSED", "0")
    mod_means, mod_calls = run()
    assert fused_means == mod_means and fused_calls == mod_calls and len(fused_means) == len(loss_lods)
    assert [c[0] for c in fused_calls] == [f"Validation/volumetric_iou/{l}" for l in loss_lods]
    record("validate_scores", only_last=int(only_last), **{f"lod{l}": s for l, s in zip(loss_lods, fused_means)})
    assert fused_means[-1] > 50.0                           # the finest LOD is the one that was fitted


def test_offline_renderer_lookat_64(monkeypatch):
    from wisp.core import Rays
    from wisp.trainers.tracker import OfflineRenderer
    from wisp.trainers.tracker.offline_renderer import _look_at
    import wisp._C as C
    pipe = fitted_pipeline()
    r = OfflineRenderer(render_res=(64, 64), shading_mode='normal', device=DEV)
    seen = []
    real = C.sdf_fd_gradient
    monkeypatch.setattr(C, "sdf_fd_gradient", lambda coords, fld, *a, **k: (seen.append(fld.get("kind")), real(coords, fld, *a, **k))[1])
    rb = r.render_lookat(pipe, f=[1.2, 0.9, 1.5], t=[0, 0, 0], fov=40.0, device=DEV)
    assert seen and set(seen) == {"hash"}                     # the normals came from wisp_hash_sdf_fd_gradient
    assert rb.rgb.shape == (64, 64, 3) and rb.hit.shape == (64, 64, 1) and rb.depth.shape == (64, 64, 1)
    assert bool(torch.isfinite(rb.rgb).all()) and float(rb.rgb.min()) >= 0.0 and float(rb.rgb.max()) <= 1.0
    hits = int(rb.hit.sum())
    assert 400 < hits < 4000
    o, d = _look_at([1.2, 0.9, 1.5], [0, 0, 0], 64, 64, fov=40.0, device=DEV)
    with torch.no_grad():
        plain = pipe.tracer(pipe.nef, rays=Rays(o, d, dist_min=0, dist_max=5)).reshape(64, 64, -1)
    assert torch.equal(rb.hit, plain.hit) and torch.equal(rb.depth, plain.depth) and torch.equal(rb.xyz, plain.xyz)
    on = rb.xyz[rb.hit[..., 0]]
    off = float((on.norm(dim=-1) - FIT["radius"]).abs().mean())
    # the shaded normals point away from the sphere's centre
    cos = float((torch.nn.functional.normalize(on, dim=-1) * (rb.rgb[rb.hit[..., 0]] * 2 - 1)).sum(-1).mean())
    record("offline_renderer", hits=hits, surface_mean_abs=off, mean_cos_normal_radius=cos)
    assert off < 0.02 and cos > 0.8


def test_train_nglod_script_end_to_end_on_a_hash_grid(tmp_path):
    """scripts/train_nglod.py --grid hash on the procedural torus with small tables for two epochs: the IoU rises, the PNGs exist"""
    out = tmp_path / "out"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "train_nglod.py"), "--write-test-mesh", str(tmp_path / "mesh"),
                        "--grid", "hash", "--codebook-bitwidth", "12", "--level", "5", "--epochs", "2", "--size", "64", "64",
                        "--out-dir", str(out)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    rec = json.loads(r.stdout.strip().splitlines()[-1])
    record("script", iou_before=rec["iou_before"], iou_after=rec["iou_after"], hits=rec["hits"], seconds=rec["seconds"])
    assert rec["grid"] == "hash" and rec["iou_after"] > rec["iou_before"]
    for name in ("render", "slice_x", "slice_y", "slice_z"):
        assert os.path.getsize(rec[name]) > 100
