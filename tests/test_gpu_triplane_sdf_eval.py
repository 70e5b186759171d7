"""GPU: the fused evaluation of a triplanar SDF field (csrc/triplane_sdf_eval.hip) - query with its IoU counters, central-difference
gradient and the fused marching iteration - against the float64 reference of tests/triplane_sdf_eval_ref.py: bit for bit on exactly
representable inputs, against the modular path's own error on generic ones, bit for bit against the two-launch marching loop - and
what is built on them: PackedSDFTracer, wisp.ops.sdf, SDFTrainer.validate, OfflineRenderer, scripts/train_nglod.py --grid triplanar.
Every measured margin is appended to profiles/triplane_sdf_eval_test_margins.jsonl when WISP_TRIPLANE_SDF_EVAL_MARGINS names a
file."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import triplane_sdf_eval_ref as R
from gpu_helpers import STATE, make_rays, march_start

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
NS = (1, 15, 17, 1000)


def record(name, **values):
    path = os.environ.get("WISP_TRIPLANE_SDF_EVAL_MARGINS")
    if path:
        with open(path, "a") as f:
            f.write(json.dumps(dict(name=name, **{k: (float(v) if not isinstance(v, (int, str)) else v) for k, v in values.items()})) + "\n")


def dev_field(fld):
    """the kernels' field dict (kind 'triplane') from a reference field, no nef in between"""
    return dict(kind='triplane', planes=[p.to(DEV).contiguous() for p in fld["planes"]], multiscale=fld["multiscale"],
                w1=fld["w1"].to(DEV).contiguous(), b1=fld["b1"].to(DEV).contiguous(), w2=fld["w2"].to(DEV).contiguous(),
                b2=fld["b2"].to(DEV).contiguous())


def nef_of(fld):
    """NeuralSDF over a TriplanarGrid (AABB) carrying a reference field's parameters; plane sizes 2^(base + l) + 1"""
    from wisp.accelstructs import AxisAlignedBBoxAS
    from wisp.models.grids import TriplanarGrid
    from wisp.models.nefs import NeuralSDF
    sizes = [int(p.shape[-1]) for p in fld["planes"][::3]]
    base = int(np.log2(sizes[0] - 1))
    assert sizes == [2 ** (base + l) + 1 for l in range(len(sizes))]
    grid = TriplanarGrid(AxisAlignedBBoxAS(), feature_dim=R.plane_features(fld), log_base_resolution=base, num_lods=len(sizes),
                         multiscale_type=fld["multiscale"], feature_std=0.01)
    nef = NeuralSDF(grid, pos_embedder='none', position_input=True, hidden_dim=fld["w1"].shape[0], num_layers=1)
    with torch.no_grad():
        for l, vol in enumerate(grid.features):
            for name, p in zip(("fmx", "fmy", "fmz"), fld["planes"][3 * l:3 * l + 3]):
                getattr(vol, name).copy_(p[None])
        nef.decoder.layers[0].weight.copy_(fld["w1"]); nef.decoder.layers[0].bias.copy_(fld["b1"])
        nef.decoder.lout.weight.copy_(fld["w2"].reshape(1, -1)); nef.decoder.lout.bias.copy_(fld["b2"])
    return nef.to(DEV).eval()


_cache = {}

# hidden 1 / 17 / 128 / 256, feature_dim 1 / 2 / 4, 'sum' of 1 and 3 levels, 'cat' of 1 and 2 levels; K = 48 as 'cat' (2 x 3 x 8) and as
# 'sum' (3 x 16); a size-1 plane (no TriplanarGrid has one: only the C entry reaches it)
EXACT = [(1, 1, 'sum', (33,)), (17, 2, 'sum', (5, 9, 17)), (128, 4, 'sum', (33,)), (256, 4, 'cat', (33,)), (128, 2, 'cat', (9, 33)),
         (17, 4, 'cat', (17, 33)), (256, 1, 'sum', (9, 17, 33)), (1, 2, 'cat', (5,)), (128, 8, 'cat', (5, 17)), (64, 16, 'sum', (9,)),
         (32, 4, 'sum', (1, 9))]


def exact(kind, hidden, F, multiscale, sizes):
    """one 1000-point exact case per key, its float64 reference computed once"""
    key = (kind, hidden, F, multiscale, sizes)
    if key not in _cache:
        if kind == "query":
            case = R.exact_case(hidden, F, multiscale, sizes, n=1000, seed=5)
            case["want"] = R.reference(case["field"], case["coords"])
        else:
            case = R.exact_gradient_case(hidden, F, multiscale, sizes, n=1000, seed=6)
            case["want"] = R.gradient_reference(case["field"], case["coords"], case["eps"])
            pos = R.offsets(case["coords"], case["eps"]).reshape(-1, 3)
            case["six"], case["want_six"] = pos, R.reference(case["field"], pos)
        case["dev"] = dev_field(case["field"])
        _cache[key] = case
    return _cache[key]


# ------------------------------------------------------------------------------------------------ 1. exact inputs
@pytest.mark.parametrize("hidden,F,multiscale,sizes", EXACT)
def test_query_equals_float64_bit_for_bit_on_exact_inputs(hidden, F, multiscale, sizes):
    import wisp._C as C
    case = exact("query", hidden, F, multiscale, sizes)
    for n in NS:
        got = C.sdf_query(case["coords"][:n].to(DEV), case["dev"])
        assert got.shape == (n, 1)
        assert torch.equal(got.double().cpu(), case["want"][:n]), (hidden, F, multiscale, sizes, n)
    assert len(torch.unique(case["want"])) > (20 if hidden > 1 else 3)      # (no dead decoder among the cases)


@pytest.mark.parametrize("hidden,F,multiscale,sizes", EXACT)
def test_gradient_equals_float64_bit_for_bit_on_exact_inputs(hidden, F, multiscale, sizes):
    """a dyadic eps: the six positions are exact points, f+ - f- and the division by 2 eps are exact.  The six values themselves
    are checked through the query at the six positions (the gradient kernel evaluates them with the same device function)."""
    import wisp._C as C
    case = exact("gradient", hidden, F, multiscale, sizes)
    six = C.sdf_query(case["six"].to(DEV), case["dev"])
    assert torch.equal(six.double().cpu(), case["want_six"])
    for n in NS:
        got = C.sdf_fd_gradient(case["coords"][:n].to(DEV), case["dev"], eps=case["eps"])
        assert got.shape == (n, 3)
        assert torch.equal(got.double().cpu(), case["want"][:n]), (hidden, F, multiscale, sizes, n)
    assert int((case["want"] != 0).sum()) > (100 if hidden > 1 else 10)


def test_empty_batch_and_python_argument_checks():
    import wisp._C as C
    case = exact("query", 17, 2, 'sum', (5, 9, 17))
    assert C.sdf_query(torch.zeros(0, 3, device=DEV), case["dev"]).shape == (0, 1)
    assert C.sdf_fd_gradient(torch.zeros(0, 3, device=DEV), case["dev"]).shape == (0, 3)
    with pytest.raises(RuntimeError, match="GPU tensor"):
        C.sdf_query(torch.zeros(4, 3), case["dev"])
    with pytest.raises(RuntimeError, match="48 feature columns"):
        C.sdf_query(torch.zeros(4, 3, device=DEV), dict(case["dev"], planes=[torch.zeros(17, 5, 5, device=DEV)] * 3,
                                                        w1=torch.zeros(17, 54, device=DEV)))


# ------------------------------------------------------------------------------------------------ 2. generic inputs
GENERIC = [(128, 4, 'sum', (33,)), (128, 4, 'sum', (9, 17, 33)), (17, 2, 'cat', (17, 33)), (256, 4, 'cat', (5, 9, 17, 33)),
           (1, 1, 'sum', (5, 9)), (128, 8, 'cat', (9, 17))]


def generic_setup(hidden, F, multiscale, sizes, n=1000):
    key = ("generic", hidden, F, multiscale, sizes)
    if key not in _cache:
        fld = R.generic_field(sizes, hidden, F=F, multiscale=multiscale, seed=3 + len(sizes), std=0.5)
        coords = R.generic_points(n, seed=9)
        _cache[key] = (fld, nef_of(fld), coords, coords.to(DEV), R.reference(fld, coords))
    return _cache[key]


@pytest.mark.parametrize("hidden,F,multiscale,sizes", GENERIC)
def test_query_error_is_within_twice_the_modular_paths(hidden, F, multiscale, sizes):
    """fused and modular path differ by roundings of the blend and of the decoder's sums only: the fused error against float64
    (same tensors) is at most twice the modular path's own - points inside the cube, on c = +-1 and outside it (reflected)"""
    from wisp.ops.sdf import fused_sdf_field
    import wisp._C as C
    fld, nef, coords, cd, want = generic_setup(hidden, F, multiscale, sizes)
    fused = fused_sdf_field(nef, None)
    assert fused is not None and fused["kind"] == "triplane" and len(fused["planes"]) == 3 * len(sizes)
    got = C.sdf_query(cd, fused).double().cpu()
    with torch.no_grad():
        mod = nef(coords=cd, channels="sdf").double().cpu()
    for name, pick in (("inside", (coords.abs() < 1).all(1)), ("face", (coords.abs() == 1).any(1) & (coords.abs() <= 1).all(1)),
                       ("outside", (coords.abs() > 1).any(1))):
        assert int(pick.sum()) > 100, name
        e_fused, e_mod = float((got - want)[pick].abs().max()), float((mod - want)[pick].abs().max())
        record("query_generic", sizes=str(sizes), hidden=hidden, F=F, multiscale=multiscale, where=name, err_fused=e_fused,
               err_modular=e_mod, fused_vs_modular=float((got - mod)[pick].abs().max()))
        print(f"{sizes} h{hidden} F{F} {multiscale} {name}: fused {e_fused:.3e} modular {e_mod:.3e}")
        assert e_fused <= 2.0 * e_mod, (name, e_fused, e_mod)


def ulps32(a, b):
    """distance of fp32 tensor a from float64 tensor b in units of the fp32 spacing at |b|"""
    spacing = torch.from_numpy(np.spacing(np.abs(b.numpy()).astype(np.float32)).astype(np.float64))
    return (a.double() - b).abs() / spacing


GRAD_MARGIN = 4.0


@pytest.mark.parametrize("hidden,F,multiscale,sizes", [GENERIC[0], GENERIC[1], GENERIC[2], GENERIC[3]])
def test_gradient_is_the_central_difference_of_the_querys_own_values(hidden, F, multiscale, sizes):
    """each component within 4 fp32 ulps of (f+ - f-) / 0.01 evaluated in float64 from wisp_triplane_sdf_query's values at
    x +- 0.005f - with the subtraction taken in float64, and with it taken in fp32 as the kernel takes it"""
    from wisp.ops.sdf import fused_sdf_field, sdf_fd_gradient
    import wisp._C as C
    fld, nef, coords, cd, _ = generic_setup(hidden, F, multiscale, sizes)
    fused = fused_sdf_field(nef, None)
    six = C.sdf_query(R.offsets(coords, 0.005).reshape(-1, 3).to(DEV), fused)[:, -1].cpu().reshape(3, 2, -1)
    diff32 = six[:, 0] - six[:, 1]                                       # the kernel's fp32 subtraction
    want = (diff32.double() / 0.01).T
    want_f64 = ((six[:, 0].double() - six[:, 1].double()) / 0.01).T
    for n in NS:
        got = sdf_fd_gradient(nef, cd[:n], None).cpu()
        u, u64 = ulps32(got, want[:n]), ulps32(got, want_f64[:n])
        record("gradient_generic", sizes=str(sizes), hidden=hidden, multiscale=multiscale, n=n, max_ulps=float(u.max()),
               max_ulps_vs_f64_difference=float(u64.max()))
        assert float(u.max()) <= GRAD_MARGIN, (n, float(u.max()))
        assert float(u64.max()) <= GRAD_MARGIN, (n, float(u64.max()))
    assert float(want.abs().max()) > 1e-3


# ------------------------------------------------------------------------------------------------ 3. IoU counters
@pytest.mark.parametrize("hidden,F,multiscale,sizes", [GENERIC[1], GENERIC[2]])
def test_iou_counts(hidden, F, multiscale, sizes):
    from wisp.ops.sdf import compute_sdf_iou
    import wisp._C as C
    fld, nef, coords, cd, want = generic_setup(hidden, F, multiscale, sizes)
    moved = dict(fld, b2=fld["b2"] - float(want.median()))               # move the output bias so that both signs occur
    dev = dev_field(moved)
    gts = R.sphere_sdf(coords, 0.9).to(DEV)
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
    record("iou_counts", sizes=str(sizes), multiscale=multiscale, n=coords.shape[0], inter=runs[0][0], union=runs[0][1])


# ------------------------------------------------------------------------------------------------ 4. one marching iteration
@pytest.mark.parametrize("hidden,F,multiscale,sizes", [GENERIC[0], GENERIC[2]])
def test_fused_marching_iteration_equals_step_then_query_bit_for_bit(hidden, F, multiscale, sizes):
    """wisp_triplane_sdf_trace_step_fused against wisp_sphere_trace_step followed by wisp_triplane_sdf_query at x of the active
    packs times scale, from a real raytrace of 300 rays against the AABB: every state array and the counter bitwise equal after
    one iteration and after 24 - both sides run the same statements"""
    import copy
    import wisp._C as C
    fld, nef, _, _, _ = generic_setup(hidden, F, multiscale, sizes)
    rays, rt, depth, st0 = march_start(nef, 300, 151)
    P = st0.t.shape[0]
    assert 100 < P <= 300
    with torch.no_grad():                                                # distances of a fraction of the cube, mostly positive
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
    record("march_exact", sizes=str(sizes), multiscale=multiscale, packs=P, active_after_24=int(b.active.sum()), hits=int(b.hit.sum()))
    assert int(b.active.sum()) < P                                         # packs left or converged


# ------------------------------------------------------------------------------------------------ 5. whole tracer
# The fit.  The march starts on the faces of the cube, so the field has to be a distance everywhere in it, not only near the surface:
# half of every batch is uniform in the cube, half lies within 0.1 of the sphere.
FIT = dict(radius=0.55, steps=400, lr=3e-3, grid_lr_weight=1.0)


def fitted_pipeline():
    """the nglod_triplanar.yaml field (TriplanarGrid 'sum', one level of three 4 x 33 x 33 planes over the AABB, hidden 128) fitted
    to the sphere of radius 0.55 with SDFTrainStep (its modular launches), with a tracer"""
    from wisp.accelstructs import AxisAlignedBBoxAS
    from wisp.models import Pipeline
    from wisp.models.grids import TriplanarGrid
    from wisp.models.nefs import NeuralSDF
    from wisp.tracers import PackedSDFTracer
    from wisp.trainers import SDFTrainStep
    if "fitted" not in _cache:
        torch.manual_seed(11)
        grid = TriplanarGrid(AxisAlignedBBoxAS(), feature_dim=4, log_base_resolution=5, num_lods=1, multiscale_type='sum',
                             feature_std=0.01)
        nef = NeuralSDF(grid, pos_embedder='none', position_input=True, hidden_dim=128, num_layers=1).to(DEV)
        step = SDFTrainStep(nef, lr=FIT["lr"], grid_lr_weight=FIT["grid_lr_weight"])
        g = torch.Generator(device=DEV).manual_seed(12)
        for _ in range(FIT["steps"]):
            xs = torch.rand(2048, 3, device=DEV, generator=g) * 2 - 1
            d = torch.nn.functional.normalize(torch.randn(1024, 3, device=DEV, generator=g), dim=1)
            xs[1024:] = d * (FIT["radius"] + 0.1 * (torch.rand(1024, 1, device=DEV, generator=g) * 2 - 1))
            step.step(xs, xs.norm(dim=-1, keepdim=True) - FIT["radius"])
        nef.eval()
        _cache["fitted"] = Pipeline(nef, PackedSDFTracer(num_steps=64, step_size=0.8, min_dis=0.0003))
    return _cache["fitted"]


def test_tracer_fused_iteration_equals_modular_marching(monkeypatch):
    """the bounds of test_sdf_tracer_fused_iteration_equals_modular_marching on a triplanar field fitted to a sphere (FIT): hit masks
    differ on at most max(2, 0.2 %) of 3000 rays, depth and xyz agree within 6e-4 (= 2 min_dis), the median depth difference is at
    most 1e-6, more than 500 hits, the surface is the sphere, and the modular march reruns bit for bit"""
    from wisp.core import Rays
    from wisp.tracers import PackedSDFTracer
    pipe = fitted_pipeline()
    nef, tracer = pipe.nef, pipe.tracer
    o, d = make_rays(3000, 151, radius=2.5, spread=0.7)
    rays = Rays(torch.from_numpy(o).to(DEV), torch.from_numpy(d).to(DEV), dist_min=0.0, dist_max=6.0)
    outs = []
    for fused in ("1", "0", "0"):
        monkeypatch.setenv("WISP_SDF_FUSED", fused)
        assert (PackedSDFTracer._fused_field(nef, 0) is not None) == (fused == "1")
        outs.append(tracer(nef, rays=rays, channels=["depth", "hit"], lod_idx=0))
    a, b, again = outs
    for name in ("hit", "depth", "xyz"):
        assert torch.equal(getattr(b, name), getattr(again, name)), name
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
    for lod in (0, None):
        fld = fused_sdf_field(nef, lod)
        assert fld is not None and fld["kind"] == "triplane"
        assert torch.equal(sdf_query(nef, cd, lod), C.sdf_query(cd, fld))
        assert torch.equal(sdf_fd_gradient(nef, cd, lod), C.sdf_fd_gradient(cd, fld, 0.005))
    counts = torch.zeros(2, dtype=torch.int64, device=DEV)
    pred = sdf_query(nef, cd, 0, gts=gts, counts=counts)
    assert counts.cpu().tolist() == [int(((pred[:, 0] < 0) & (gts < 0)).sum()), int(((pred[:, 0] < 0) | (gts < 0)).sum())]
    with torch.no_grad():
        diff = float((pred - nef(coords=cd, lod_idx=0, channels="sdf")).abs().max())
    record("public_query", fused_vs_modular=diff)
    assert diff <= 1e-5
    # a broken rule falls back to the module, exactly: a 'cat' field below its last level, and the switch
    _, cat, _, _, _ = generic_setup(*GENERIC[2])
    assert fused_sdf_field(cat, 1) is not None and fused_sdf_field(cat, 0) is None
    monkeypatch.setenv("WISP_SDF_FUSED", "0")
    assert fused_sdf_field(nef, 0) is None
    counts.zero_()
    with torch.no_grad():
        pred = sdf_query(nef, cd, 0, gts=gts, counts=counts)
        assert torch.equal(pred, nef(coords=cd, lod_idx=0, channels="sdf"))
        assert torch.equal(sdf_fd_gradient(nef, cd, 0), finitediff_gradient(cd, lambda x: nef(coords=x, lod_idx=0, channels="sdf")))
    assert counts.cpu().tolist() == [int(((pred[:, 0] < 0) & (gts < 0)).sum()), int(((pred[:, 0] < 0) | (gts < 0)).sum())]
    assert sdf_query(nef, cd[:0], 0).shape == (0, 1) and sdf_fd_gradient(nef, cd[:0], 0).shape == (0, 3)      # empty batches
    monkeypatch.setenv("WISP_SDF_FUSED", "1")
    assert sdf_query(nef, cd[:0], 0).shape == (0, 1) and sdf_fd_gradient(nef, cd[:0], 0).shape == (0, 3)


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


def test_validate_fused_equals_modular(monkeypatch):
    """SDFTrainer.validate() through one launch per batch against WISP_SDF_FUSED=0 over the same batches: the counters are integers,
    so the scores are EQUAL unless a prediction sits within the fused-vs-modular difference of 0 - asserted per batch"""
    from wisp.ops.sdf import sdf_query
    from wisp.trainers import ConfigAdam, ConfigDataloader, ConfigSDFTrainer, SDFTrainer
    pipe = fitted_pipeline()
    nef = pipe.nef
    ds = _SphereSet(1000, 21)
    monkeypatch.setattr(SDFTrainer, "_validation_metric_name", lambda self: "volumetric_iou")
    cfg = ConfigSDFTrainer(optimizer=ConfigAdam(lr=1e-3, eps=1e-15), dataloader=ConfigDataloader(batch_size=300), max_epochs=1,
                           only_last=True, profile_nvtx=False)
    trainer = SDFTrainer(cfg, pipe, ds, device=DEV)
    torch.manual_seed(77)
    batches = list(trainer.train_data_loader)                 # one seeded pass, then the same batches for both runs
    assert [b["coords"].shape[0] for b in batches] == [300, 300, 300, 100]
    trainer.train_data_loader = _FixedLoader(batches)
    for bi, b in enumerate(batches):
        with torch.no_grad():
            pm = nef(coords=b["coords"], lod_idx=0, channels="sdf").reshape(-1)
        pf = sdf_query(nef, b["coords"], 0).reshape(-1)
        diff = float((pf - pm).abs().max())
        near = int((pm.abs() <= diff).sum())
        record("validate", batch=bi, fused_vs_modular=diff, min_abs_pred=float(pm.abs().min()), near=near)
        assert near == 0, (bi, diff, float(pm.abs().min()))

    def run():
        calls = []
        monkeypatch.setattr(trainer.tracker, "log_metric", lambda *a, **k: calls.append(a), raising=False)
        return trainer.validate()["volumetric_iou"], calls
    fused_means, fused_calls = run()
    monkeypatch.setenv("WISP_SDF_FUSED", "0")
    mod_means, mod_calls = run()
    assert fused_means == mod_means and fused_calls == mod_calls and len(fused_means) == 1
    assert [c[0] for c in fused_calls] == ["Validation/volumetric_iou/0"]
    record("validate_scores", lod0=fused_means[0])
    assert fused_means[-1] > 50.0


def test_tracer_default_is_unchanged_and_fused_normals_agree():
    """fused_normals unset == explicitly False, bit for bit; set, the march (hit, depth, xyz) is identical and the unit normals
    agree with the six-query ones (both difference the same field; the fused values differ from the modular ones by rounding)"""
    from wisp.core import Rays
    from wisp.trainers.tracker.offline_renderer import _look_at
    pipe = fitted_pipeline()
    o, d = _look_at([1.2, 0.9, 1.5], [0, 0, 0], 32, 32, fov=40.0, device=DEV)
    tracer = pipe.tracer
    assert not hasattr(tracer, "fused_normals")

    def trace():
        with torch.no_grad():
            return tracer(pipe.nef, rays=Rays(o, d, dist_min=0.0, dist_max=6.0))
    base = trace()
    tracer.fused_normals = False
    off = trace()
    for name in ("hit", "depth", "xyz", "normal", "rgb", "alpha"):
        assert torch.equal(getattr(base, name), getattr(off, name)), name
    tracer.fused_normals = True
    on = trace()
    del tracer.fused_normals
    for name in ("hit", "depth", "xyz", "alpha"):
        assert torch.equal(getattr(base, name), getattr(on, name)), name
    hit = base.hit.reshape(-1)
    assert int(hit.sum()) > 100
    cos = (base.normal.reshape(-1, 3)[hit] * on.normal.reshape(-1, 3)[hit]).sum(-1)
    record("fused_normals", hits=int(hit.sum()), min_cos=float(cos.min()))
    assert float(cos.min()) > 0.999


@pytest.mark.parametrize("mode", ["rb", "normal", "matcap"])
def test_offline_renderer_lookat_64(mode, monkeypatch, tmp_path):
    from wisp.core import Rays
    from wisp.ops.image import save_u8
    from wisp.trainers.tracker import OfflineRenderer
    from wisp.trainers.tracker.offline_renderer import _look_at
    import wisp._C as C
    pipe = fitted_pipeline()
    ys, xs = np.meshgrid(np.arange(48), np.arange(64), indexing='ij')
    matcap = str(tmp_path / "matcap.png")
    save_u8(matcap, np.stack([xs * 4, ys * 5, 255 - xs * 3], -1).clip(0, 255).astype(np.uint8))
    r = OfflineRenderer(render_res=(64, 64), shading_mode=mode, matcap_path=matcap, device=DEV)
    seen = []
    real = C.sdf_fd_gradient
    monkeypatch.setattr(C, "sdf_fd_gradient", lambda coords, fld, *a, **k: (seen.append(fld.get("kind")), real(coords, fld, *a, **k))[1])
    rb = r.render_lookat(pipe, f=[1.2, 0.9, 1.5], t=[0, 0, 0], fov=40.0, device=DEV)
    assert seen and set(seen) == {"triplane"}                 # the normals came from wisp_triplane_sdf_fd_gradient
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
    record("offline_renderer", mode=mode, hits=hits, surface_mean_abs=off)
    assert off < 0.02
    if mode == "normal":                                      # the shaded normals point away from the sphere's centre
        cos = float((torch.nn.functional.normalize(on, dim=-1) * (rb.rgb[rb.hit[..., 0]] * 2 - 1)).sum(-1).mean())
        assert cos > 0.8


def test_train_nglod_script_end_to_end_on_a_triplanar_grid(tmp_path):
    """scripts/train_nglod.py --grid triplanar on the procedural torus for two epochs: the field took the fused kernels, the IoU
    rises, the PNGs exist"""
    out = tmp_path / "out"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "train_nglod.py"), "--write-test-mesh", str(tmp_path / "mesh"),
                        "--grid", "triplanar", "--epochs", "2", "--num-samples", "50000", "--size", "64", "64", "--out-dir", str(out)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    rec = json.loads(r.stdout.strip().splitlines()[-1])
    record("script", iou_before=rec["iou_before"], iou_after=rec["iou_after"], hits=rec["hits"], seconds=rec["seconds"])
    assert rec["grid"] == "triplanar" and rec["dataset"] == "mesh" and rec["fused_triplane_eval"] is True
    assert rec["iou_after"] > rec["iou_before"]
    for name in ("render", "slice_x", "slice_y", "slice_z"):
        assert os.path.getsize(rec[name]) > 100
