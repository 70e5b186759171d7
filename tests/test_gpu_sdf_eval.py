"""GPU: the fused nglod field query, its IoU counters and central-difference gradient (csrc/sdf_eval.hip) against the float64
reference of tests/sdf_eval_ref.py - bit for bit on exactly representable inputs, against the modular path's own error on generic
ones - and what is built on them: wisp.ops.sdf, the tracer's fused normals, SDFTrainer.validate, OfflineRenderer, the nglod script.
Every measured margin is appended to profiles/sdf_eval_test_margins.jsonl when WISP_SDF_EVAL_MARGINS names a file."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import sdf_eval_ref as R
from gpu_helpers import STATE, march_start

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
NS = (1, 15, 17, 1000)
LEVELS = {"last": (2, 3, 4), "middle": (2, 3)}


def record(name, **values):
    path = os.environ.get("WISP_SDF_EVAL_MARGINS")
    if path:
        with open(path, "a") as f:
            f.write(json.dumps(dict(name=name, **{k: (float(v) if not isinstance(v, (int, str)) else v) for k, v in values.items()})) + "\n")


def dev_field(sh, fld):
    """the kernel's tensors from a reference field and the shell's oracle structures (no nef in between)"""
    cu = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a)).to(dt).to(DEV)
    return dict(feats=[f.to(DEV).contiguous() for f in fld["feats"]], levels=list(fld["levels"]), half_round=fld["half_round"],
                w1=fld["w1"].to(DEV).contiguous(), b1=fld["b1"].to(DEV).contiguous(), w2=fld["w2"].to(DEV).contiguous(),
                b2=fld["b2"].to(DEV).contiguous(), octree=cu(sh.octree, torch.uint8), exsum=cu(sh.exsum, torch.int32),
                points=cu(sh.points, torch.int16), trinkets=cu(sh.trinkets, torch.int32))


def make_nef(sh, levels_all=(2, 3, 4), hidden=128, tex=False, pos=True, seed=3, half=True, std=0.05, positional=False):
    """NeuralSDF / NeuralSDFTex over an OctreeGrid on the shell's cells"""
    from wisp.accelstructs import OctreeAS
    from wisp.models.grids import OctreeGrid
    from wisp.models.nefs.neural_sdf import NeuralSDF
    from wisp.models.nefs.neural_sdf_tex import NeuralSDFTex
    torch.manual_seed(seed)
    blas = OctreeAS.from_quantized_points(torch.from_numpy(sh.cells).short().to(DEV), sh.level)
    grid = OctreeGrid(blas, feature_dim=16, num_lods=len(levels_all), multiscale_type='sum', feature_std=std)
    grid.half_features = half
    if tex:
        nef = NeuralSDFTex(grid, embedder_type='identity' if pos else 'none', hidden_dim=hidden, num_layers=1)
    else:
        nef = NeuralSDF(grid, pos_embedder='positional' if positional else 'none', position_input=True, hidden_dim=hidden, num_layers=1)
    nef = nef.to(DEV)
    assert list(grid.active_lods) == list(levels_all)
    return nef


def ref_field_of(nef, lod_idx):
    """the reference's view (CPU tensors) of a nef's parameters at lod_idx; textured without position: zero position columns"""
    g, dec = nef.grid, nef.decoder
    w1 = dec.layers[0].weight.detach().float().cpu()
    if w1.shape[1] == 16:
        w1 = torch.cat([torch.zeros(w1.shape[0], 3), w1], 1)
    return dict(levels=tuple(g.active_lods[:lod_idx + 1]), feats=[g.features[i].detach().cpu() for i in range(lod_idx + 1)],
                half_round=bool(g.half_features), w1=w1, b1=dec.layers[0].bias.detach().float().cpu(),
                w2=dec.lout.weight.detach().float().cpu(), b2=dec.lout.bias.detach().float().cpu())


def modular_raw(nef, coords, lod_idx):
    """the raw decoder outputs through the modular ops, [n, rows]"""
    from wisp.models.nefs.neural_sdf_tex import NeuralSDFTex
    with torch.no_grad():
        if type(nef) is NeuralSDFTex:
            feats = nef.grid.interpolate(coords, lod_idx)
            if nef.position_input:
                feats = torch.cat([nef.pos_embedder(coords), feats], dim=-1)
            return nef.decoder(feats).float()
        return nef(coords=coords, lod_idx=lod_idx, channels="sdf").float()


_exact = {}


def exact(kind, lods, hidden, rows, dtype=torch.float32, half=False):
    """one 1000-point exact case per key, its float64 reference computed once"""
    key = (kind, lods, hidden, rows, dtype, half)
    if key not in _exact:
        if kind == "query":
            case = R.exact_case(LEVELS[lods], hidden, rows, n=1000, b=1, seed=5, dtype=dtype, half_round=half)
            case["want"] = R.reference(case["shell"], case["field"], case["coords"])
        else:
            case = R.exact_gradient_case(LEVELS[lods], hidden, rows, n=1000, seed=6, dtype=dtype)
            case["want"] = R.gradient_reference(case["shell"], case["field"], case["coords"], case["eps"])
            pos = R.offsets(case["coords"], case["eps"]).reshape(-1, 3)
            case["six"], case["want_six"] = pos, R.reference(case["shell"], case["field"], pos)
        case["dev"] = dev_field(case["shell"], case["field"])
        _exact[key] = case
    return _exact[key]


# ------------------------------------------------------------------------------------------------ exact inputs
@pytest.mark.parametrize("lods", ["last", "middle"])
@pytest.mark.parametrize("rows", [1, 4])
@pytest.mark.parametrize("hidden", [1, 17, 128, 256])
def test_query_equals_float64_bit_for_bit_on_exact_inputs(hidden, rows, lods):
    import wisp._C as C
    case = exact("query", lods, hidden, rows)
    for n in NS:
        got = C.sdf_query(case["coords"][:n].to(DEV), case["dev"])
        assert got.shape == (n, rows)
        assert torch.equal(got.double().cpu(), case["want"][:n]), (hidden, rows, lods, n)
    assert int((case["chain"] < 0).sum()) > 100 and int((case["want"] != 0).sum()) > 250     # misses and live values both present


@pytest.mark.parametrize("dtype,half", [(torch.float32, True), (torch.float16, False), (torch.float16, True), (torch.bfloat16, False)])
@pytest.mark.parametrize("rows", [1, 4])
def test_query_exact_over_table_dtypes_and_half_rounding(rows, dtype, half):
    import wisp._C as C
    case = exact("query", "last", 128, rows, dtype, half)
    for n in NS:
        got = C.sdf_query(case["coords"][:n].to(DEV), case["dev"])
        assert torch.equal(got.double().cpu(), case["want"][:n]), (rows, dtype, half, n)


@pytest.mark.parametrize("lods", ["last", "middle"])
@pytest.mark.parametrize("rows", [1, 4])
@pytest.mark.parametrize("hidden", [1, 17, 128, 256])
def test_gradient_equals_float64_bit_for_bit_on_exact_inputs(hidden, rows, lods):
    """eps = 2^-6: the six positions are exact points, f+ - f- and the division by 2^-5 are exact.  The six values themselves are
    checked through the query at the six positions (the gradient kernel evaluates them with the same device function)."""
    import wisp._C as C
    case = exact("gradient", lods, hidden, rows)
    six = C.sdf_query(case["six"].to(DEV), case["dev"])
    assert torch.equal(six.double().cpu(), case["want_six"])
    for n in NS:
        got = C.sdf_fd_gradient(case["coords"][:n].to(DEV), case["dev"], eps=case["eps"])
        assert got.shape == (n, 3)
        assert torch.equal(got.double().cpu(), case["want"][:n]), (hidden, rows, lods, n)
    assert int((case["want"] != 0).sum()) > 500


def test_empty_batch_and_python_argument_checks():
    import wisp._C as C
    case = exact("query", "last", 17, 1)
    assert C.sdf_query(torch.zeros(0, 3, device=DEV), case["dev"]).shape == (0, 1)
    assert C.sdf_fd_gradient(torch.zeros(0, 3, device=DEV), case["dev"]).shape == (0, 3)
    with pytest.raises(RuntimeError, match="GPU tensor"):
        C.sdf_query(torch.zeros(4, 3), case["dev"])


# ------------------------------------------------------------------------------------------------ generic inputs
GENERIC = [("sdf", 128, True, torch.float32, 2), ("sdf", 128, False, torch.float32, 1), ("sdf", 17, True, torch.float32, 2),
           ("tex_pos", 128, True, torch.float32, 2), ("tex", 128, True, torch.float32, 1), ("tex_pos", 256, False, torch.float32, 2),
           ("sdf", 128, True, torch.float16, 2), ("tex_pos", 128, False, torch.float16, 2)]


def generic_setup(kind, hidden, half, dtype, lod_idx, n=1000):
    sh = R.shell(4)
    nef = make_nef(sh, hidden=hidden, tex=kind != "sdf", pos=kind != "tex", half=half)
    if dtype != torch.float32:
        for f in nef.grid.features:
            f.data = f.data.to(dtype)
    coords = R.generic_points(n, seed=9)
    return sh, nef, coords, coords.to(DEV)


@pytest.mark.parametrize("kind,hidden,half,dtype,lod_idx", GENERIC)
def test_query_error_is_within_twice_the_modular_paths(kind, hidden, half, dtype, lod_idx):
    """fused and modular path differ by summation order only: the fused error against float64 (same fp32 tensors) is at most twice
    the modular path's own, on every output row"""
    from wisp.ops.sdf import fused_sdf_field
    import wisp._C as C
    sh, nef, coords, cd = generic_setup(kind, hidden, half, dtype, lod_idx)
    fld = fused_sdf_field(nef, lod_idx)
    assert fld is not None and fld["b2"].numel() == (1 if kind == "sdf" else 4)
    want = R.reference(sh, ref_field_of(nef, lod_idx), coords)
    got = C.sdf_query(cd, fld).double().cpu()
    if dtype == torch.float32:
        mod = modular_raw(nef, cd, lod_idx).double().cpu()
    else:
        # the modular ops take 16-bit tables only under autocast; the same tables as fp32 values give the same numbers
        twin = make_nef(sh, hidden=hidden, tex=kind != "sdf", pos=kind != "tex", half=half)
        twin.load_state_dict({k: v.float() for k, v in nef.state_dict().items()})
        mod = modular_raw(twin, cd, lod_idx).double().cpu()
    for r in range(want.shape[1]):
        e_fused, e_mod = float((got[:, r] - want[:, r]).abs().max()), float((mod[:, r] - want[:, r]).abs().max())
        record("query_generic", kind=kind, hidden=hidden, half=int(half), dtype=str(dtype), lod_idx=lod_idx, row=r,
               err_fused=e_fused, err_modular=e_mod, fused_vs_modular=float((got[:, r] - mod[:, r]).abs().max()))
        print(f"{kind} h{hidden} half{int(half)} {dtype} lod{lod_idx} row{r}: fused {e_fused:.3e} modular {e_mod:.3e}")
        assert e_fused <= 2.0 * e_mod, (kind, hidden, half, dtype, lod_idx, r, e_fused, e_mod)


@pytest.mark.parametrize("kind,hidden,lod_idx", [("sdf", 128, 2), ("tex_pos", 128, 1)])
def test_iou_counts(kind, hidden, lod_idx):
    from wisp.ops.sdf import fused_sdf_field, compute_sdf_iou
    import wisp._C as C
    sh, nef, coords, cd = generic_setup(kind, hidden, True, torch.float32, lod_idx)
    with torch.no_grad():                                 # move the distance bias so that both signs occur
        nef.decoder.lout.bias[-1] -= float(modular_raw(nef, cd, lod_idx)[:, -1].median())
    fld = fused_sdf_field(nef, lod_idx)
    gts = R.sphere_sdf(coords).to(DEV)
    runs = []
    for _ in range(3):
        counts = torch.zeros(2, dtype=torch.int64, device=DEV)
        out = C.sdf_query(cd, fld, gts=gts, counts=counts)
        runs.append(counts.cpu().tolist())
    pred = out[:, -1]
    same_launch = [int(((pred < 0) & (gts < 0)).sum()), int(((pred < 0) | (gts < 0)).sum())]
    assert runs[0] == same_launch and runs[1] == runs[0] and runs[2] == runs[0]
    only = torch.zeros(2, dtype=torch.int64, device=DEV)
    assert C.sdf_query(cd, fld, gts=gts, counts=only, with_out=False) is None and only.cpu().tolist() == runs[0]
    assert 0 < runs[0][0] < runs[0][1] < coords.shape[0]
    # against the reference's metric on the modular prediction: points whose modular |pred| lies below the fused-vs-modular
    # difference may fall on either side
    mod = modular_raw(nef, cd, lod_idx)[:, -1]
    diff = float((pred - mod).abs().max())
    cap = int((mod.abs() <= diff).sum())
    inter_m, union_m = int(((mod < 0) & (gts < 0)).sum()), int(((mod < 0) | (gts < 0)).sum())
    record("iou_counts", kind=kind, fused_vs_modular=diff, cap=cap, n=coords.shape[0], inter=runs[0][0], union=runs[0][1],
           inter_modular=inter_m, union_modular=union_m)
    assert cap < 0.01 * coords.shape[0]
    assert abs(runs[0][0] - inter_m) <= cap and abs(runs[0][1] - union_m) <= cap
    assert abs(100.0 * runs[0][0] / runs[0][1] - compute_sdf_iou(mod[:, None], gts[:, None])) <= 100.0 * 2 * (cap + 1e-9) / union_m + 1e-9
    # accumulation: a second batch adds to the same counters
    C.sdf_query(cd[:17], fld, gts=gts[:17], counts=only, with_out=False)
    extra = [int(((pred[:17] < 0) & (gts[:17] < 0)).sum()), int(((pred[:17] < 0) | (gts[:17] < 0)).sum())]
    assert only.cpu().tolist() == [runs[0][0] + extra[0], runs[0][1] + extra[1]]


def ulps32(a, b):
    """distance of fp32 tensor a from float64 tensor b in units of the fp32 spacing at |b|"""
    spacing = torch.from_numpy(np.spacing(np.abs(b.numpy()).astype(np.float32)).astype(np.float64))
    return (a.double() - b).abs() / spacing


GRAD_MARGIN = 4.0


@pytest.mark.parametrize("kind,hidden,lod_idx", [("sdf", 128, 2), ("sdf", 17, 1), ("tex_pos", 128, 2), ("tex", 256, 2)])
def test_gradient_is_the_central_difference_of_the_querys_own_values(kind, hidden, lod_idx):
    """each component within 4 fp32 ulps of (f+ - f-) / 0.01 evaluated in float64 from wisp_sdf_query's values at x +- 0.005f -
    with the subtraction taken in float64, and with it taken in fp32 as the kernel takes it (one division rounding + the fp32 /
    fp64 representation of 0.01; f+ and f- are the query's, bit for bit)"""
    from wisp.ops.sdf import fused_sdf_field, sdf_fd_gradient
    import wisp._C as C
    sh, nef, coords, cd = generic_setup(kind, hidden, True, torch.float32, lod_idx)
    fld = fused_sdf_field(nef, lod_idx)
    six = C.sdf_query(R.offsets(coords, 0.005).reshape(-1, 3).to(DEV), fld)[:, -1].cpu().reshape(3, 2, -1)
    diff32 = six[:, 0] - six[:, 1]                                       # the kernel's fp32 subtraction
    want = (diff32.double() / 0.01).T
    want_f64 = ((six[:, 0].double() - six[:, 1].double()) / 0.01).T
    for n in NS:
        got = sdf_fd_gradient(nef, cd[:n], lod_idx).cpu()
        u, u64 = ulps32(got, want[:n]), ulps32(got, want_f64[:n])
        record("gradient_generic", kind=kind, hidden=hidden, lod_idx=lod_idx, n=n, max_ulps=float(u.max()),
               max_ulps_vs_f64_difference=float(u64.max()))
        assert float(u.max()) <= GRAD_MARGIN, (kind, n, float(u.max()))
        assert float(u64.max()) <= GRAD_MARGIN, (kind, n, float(u64.max()))
    assert float(want.abs().max()) > 1e-3


# ------------------------------------------------------------------------------------------------ one marching iteration
@pytest.mark.parametrize("kind,hidden,half,dtype,lod_idx", [("sdf", 128, True, torch.float32, 2), ("sdf", 17, False, torch.float16, 1),
                                                            ("tex_pos", 128, True, torch.float32, 2)])
def test_fused_marching_iteration_equals_step_then_query_bit_for_bit(kind, hidden, half, dtype, lod_idx):
    """wisp_sdf_trace_step_fused against wisp_sphere_trace_step followed by wisp_sdf_query at x of the active packs times scale,
    from a real raytrace of 300 rays through the level-4 shell: every state array bitwise equal after the first launch and after
    each of 24 iterations - both sides run sphere_trace_step and sdf_eval_point.  A textured field marches on row 3 of its output
    layer (PackedSDFTracer._fused_field_tex); its query side takes column 3 of the four-row field."""
    import copy
    from wisp.ops.sdf import fused_sdf_field
    from wisp.tracers import PackedSDFTracer
    import wisp._C as C
    sh, nef, _, _ = generic_setup(kind, hidden, half, dtype, lod_idx, n=1)
    rays, rt, depth, st0 = march_start(nef, 300, 151)
    P = st0.t.shape[0]
    assert 100 < P <= 300
    march = PackedSDFTracer._fused_field(nef, lod_idx)
    rows = fused_sdf_field(nef, lod_idx)
    assert march is not None and march["b2"].numel() == 1 and rows["b2"].numel() == (1 if kind == "sdf" else 4)
    v = C.sdf_query(st0.x, march)                                        # distances of about a cell's size, mostly positive
    march = dict(march, b2=march["b2"] - float(v.median()) + 0.15)
    b2 = rows["b2"].clone()
    b2[-1] = march["b2"][0]
    rows = dict(rows, b2=b2)
    scale, min_dis, dist_max = 0.8, 0.0003, float(rays.dist_max)
    a, b = copy.deepcopy(st0), copy.deepcopy(st0)
    counter = torch.zeros(1, dtype=torch.int32, device=DEV)

    def fused(st, first, cnt=None):
        C.sdf_trace_step_field(first, st.o, st.d, depth, rt.pidx, dist_max, min_dis, min_dis * 5, st.t, st.dist, st.dist_prev,
                               st.active, st.hit, st.nug, st.nug_next, st.cell, st.x, march, scale, cnt)

    def query(st):
        sel = st.active.bool()
        if bool(sel.any()):
            st.dist[sel] = C.sdf_query(st.x[sel], rows)[:, -1] * scale

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
    record("march_exact", kind=kind, hidden=hidden, half=int(half), dtype=str(dtype), lod_idx=lod_idx, packs=P,
           active_after_24=int(b.active.sum()), hits=int(b.hit.sum()), moved_cells=moved)
    assert int(b.active.sum()) < P and moved > 10                          # packs left or converged, and cells were jumped


# ------------------------------------------------------------------------------------------------ fallback
def test_unsupported_field_falls_back_to_the_modular_path_exactly(monkeypatch):
    from wisp.ops.differential import finitediff_gradient
    from wisp.ops.sdf import fused_sdf_field, sdf_query, sdf_fd_gradient
    sh = R.shell(4)
    cd = R.generic_points(300, seed=2).to(DEV)
    nef = make_nef(sh, positional=True)                       # a Fourier position embedding: not the fused shape
    assert fused_sdf_field(nef, 2) is None
    with torch.no_grad():
        assert torch.equal(sdf_query(nef, cd, 2), nef(coords=cd, lod_idx=2, channels="sdf"))
        assert torch.equal(sdf_fd_gradient(nef, cd, 2), finitediff_gradient(cd, lambda x: nef(coords=x, lod_idx=2, channels="sdf")))
    ok = make_nef(sh)
    assert fused_sdf_field(ok, 2) is not None and fused_sdf_field(ok, 0) is None
    counts = torch.zeros(2, dtype=torch.int64, device=DEV)
    gts = R.sphere_sdf(cd.cpu()).to(DEV)
    monkeypatch.setenv("WISP_SDF_FUSED", "0")
    assert fused_sdf_field(ok, 2) is None
    with torch.no_grad():
        pred = sdf_query(ok, cd, 2, gts=gts, counts=counts)
        assert torch.equal(pred, ok(coords=cd, lod_idx=2, channels="sdf"))
    assert counts.cpu().tolist() == [int(((pred[:, 0] < 0) & (gts < 0)).sum()), int(((pred[:, 0] < 0) | (gts < 0)).sum())]
    tex = make_nef(sh, tex=True, pos=True)
    with torch.no_grad():
        rgb, sdf = tex(coords=cd, lod_idx=2, channels=["rgb", "sdf"])
        assert torch.equal(sdf_query(tex, cd, 2), torch.cat([rgb, sdf], -1))


# ------------------------------------------------------------------------------------------------ what is built on the kernels
def fitted_pipeline(tex=False, steps=150):
    """a field on the shell's cells briefly fitted to the sphere of radius 0.625 (which runs through the shell), with a tracer"""
    from wisp.models import Pipeline
    from wisp.tracers import PackedSDFTracer
    from wisp.trainers import SDFTrainStep
    key = ("fitted", tex)
    if key not in _exact:
        sh = R.shell(4)
        nef = make_nef(sh, tex=tex, pos=True, seed=11, std=0.01)
        g = torch.Generator().manual_seed(4)
        step = SDFTrainStep(nef, lr=5e-3)
        for _ in range(steps):
            d = torch.nn.functional.normalize(torch.randn(512, 3, generator=g), dim=1)
            pts = (d * (0.625 + 0.12 * torch.randn(512, 1, generator=g))).to(DEV)
            gts = (pts.norm(dim=1, keepdim=True) - 0.625)
            step.step(pts, gts, *((0.5 + 0.5 * torch.nn.functional.normalize(pts, dim=1),) if tex else ()))
        nef.eval()
        _exact[key] = Pipeline(nef, PackedSDFTracer(num_steps=64, step_size=0.8, min_dis=0.0003))
    return _exact[key]


class _ShellSet:
    """stand-in for a mesh dataset: points around the sphere with their distances, served in batches by get_batch"""

    def __init__(self, n, seed):
        g = torch.Generator().manual_seed(seed)
        d = torch.nn.functional.normalize(torch.randn(n, 3, generator=g), dim=1)
        self.coords = (d * (0.625 + 0.1 * torch.randn(n, 1, generator=g))).to(DEV)
        self.sdf = self.coords.norm(dim=1, keepdim=True) - 0.625
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


@pytest.mark.parametrize("only_last", [True, False])
def test_validate_fused_against_modular(only_last, monkeypatch):
    """SDFTrainer.validate(), one launch per batch and fused LOD, against WISP_SDF_FUSED=0 over the batches of one seeded pass of
    the loader.  Per batch and LOD: the integer counts of the fused launch differ from the modular prediction's by at most the
    number of points whose modular |pred| lies within the MEASURED fused-vs-modular difference of that batch at that LOD (under
    1 % of the batch); the scores validate() logs and returns are those counts' IoUs; a LOD outside the fused shape is exact."""
    import wisp.trainers.sdf_trainer as mod
    from wisp.ops.sdf import sdf_query
    from wisp.trainers import ConfigAdam, ConfigDataloader, ConfigSDFTrainer, SDFTrainer
    pipe = fitted_pipeline()
    nef = pipe.nef
    ds = _ShellSet(1000, 21)
    monkeypatch.setattr(SDFTrainer, "_validation_metric_name", lambda self: "volumetric_iou")
    cfg = ConfigSDFTrainer(optimizer=ConfigAdam(lr=1e-3, eps=1e-15), dataloader=ConfigDataloader(batch_size=300), max_epochs=1,
                           only_last=only_last, profile_nvtx=False)
    trainer = SDFTrainer(cfg, pipe, ds, device=DEV)
    torch.manual_seed(77)
    batches = list(trainer.train_data_loader)                 # one seeded pass, then the same batches for both runs
    assert [b["coords"].shape[0] for b in batches] == [300, 300, 300, 100]
    trainer.train_data_loader = _FixedLoader(batches)
    loss_lods = [2] if only_last else [0, 1, 2]
    fused_lods = [l for l in loss_lods if l >= 1]             # (LOD index 0 is outside the fused shape and stays modular)

    def run():
        calls, rows = [], []
        monkeypatch.setattr(trainer.tracker, "log_metric", lambda *a, **k: calls.append(a), raising=False)
        real = mod._hip().sdf_query
        monkeypatch.setattr(mod._hip(), "sdf_query", lambda *a, **k: (rows.append(k["counts"]), real(*a, **k))[1])
        out = trainer.validate()
        monkeypatch.setattr(mod._hip(), "sdf_query", real)
        return out["volumetric_iou"], calls, [r.cpu().tolist() for r in rows]
    fused_means, fused_calls, fused_counts = run()
    assert len(fused_counts) == len(batches) * len(fused_lods)
    monkeypatch.setenv("WISP_SDF_FUSED", "0")
    mod_means, mod_calls, none = run()
    assert none == []
    monkeypatch.delenv("WISP_SDF_FUSED")
    scores_f, scores_m = [], []
    it = iter(fused_counts)
    for bi, b in enumerate(batches):
        pts, gts = b["coords"], b["sdf"].reshape(-1)
        for lod in loss_lods:
            with torch.no_grad():
                pm = nef(coords=pts, lod_idx=lod, channels="sdf").reshape(-1)
            im, um = int(((pm < 0) & (gts < 0)).sum()), int(((pm < 0) | (gts < 0)).sum())
            scores_m.append(100.0 * (im / um))
            if lod not in fused_lods:
                scores_f.append(scores_m[-1])
                continue
            pf = sdf_query(nef, pts, lod).reshape(-1)
            diff = float((pf - pm).abs().max())
            cap = int((pm.abs() <= diff).sum())
            i_f, u_f = next(it)
            record("validate", only_last=int(only_last), batch=bi, lod=lod, n=int(pts.shape[0]), fused_vs_modular=diff, cap=cap,
                   inter=i_f, union=u_f, inter_modular=im, union_modular=um)
            assert cap < 0.01 * pts.shape[0], (bi, lod, cap)
            assert abs(i_f - im) <= cap and abs(u_f - um) <= cap, (bi, lod, (i_f, u_f), (im, um), cap)
            assert [i_f, u_f] == [int(((pf < 0) & (gts < 0)).sum()), int(((pf < 0) | (gts < 0)).sum())]
            scores_f.append(100.0 * (i_f / u_f))
    n = len(loss_lods)
    # what validate() logs (the first len(loss_lods) scores, the reference's zip) and returns (the mean over the batches per LOD)
    assert [c[1] for c in fused_calls] == scores_f[:n] and [c[1] for c in mod_calls] == scores_m[:n]
    assert [c[0] for c in fused_calls] == [f"Validation/volumetric_iou/{l}" for l in loss_lods] == [c[0] for c in mod_calls]
    assert fused_means == [sum(scores_f[i::n]) / len(batches) for i in range(n)]
    assert mod_means == [sum(scores_m[i::n]) / len(batches) for i in range(n)]
    assert fused_means[-1] > 50.0                           # the finest LOD is the one that was fitted


def test_tracer_default_is_unchanged_and_fused_normals_agree():
    """fused_normals unset == explicitly False, bit for bit; set, the march (hit, depth, xyz) is identical and the unit normals
    agree to the gradient margin"""
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
    hits = int(base.hit.sum())
    assert 100 < hits < 1000
    err = float((on.normal - base.normal)[base.hit].abs().max())
    # the two gradients differ by the fused-vs-modular difference d of the six distances, 2 d / 0.01 per component, plus
    # GRAD_MARGIN ulps; normalising a gradient of length >= gmin divides that by gmin (and at most doubles it)
    from wisp.ops.differential import finitediff_gradient
    from wisp.ops.sdf import sdf_query
    x = base.xyz[base.hit]
    pos = R.offsets(x.cpu(), 0.005).reshape(-1, 3).to(DEV)
    with torch.no_grad():
        d = float((sdf_query(pipe.nef, pos) - pipe.nef(coords=pos, channels="sdf")).abs().max())
        g = finitediff_gradient(x, pipe.nef.get_forward_function("sdf"))
    gmin, gmax = float(g.norm(dim=1).min()), float(g.abs().max())
    bound = 2.0 * (2.0 * d / 0.01 + GRAD_MARGIN * 2.0 ** -23 * gmax) / gmin
    record("tracer_normals", hits=hits, max_abs_diff=err, fused_vs_modular=d, gmin=gmin, bound=bound)
    assert gmin > 0.1 and err <= bound, (err, bound)


@pytest.mark.parametrize("mode,tex", [("rb", False), ("normal", False), ("matcap", False), ("rb", True)])
def test_offline_renderer_modes(mode, tex, tmp_path):
    from wisp.ops.image import save_u8
    from wisp.trainers.tracker import OfflineRenderer
    pipe = fitted_pipeline(tex=tex)
    ys, xs = np.meshgrid(np.arange(48), np.arange(64), indexing='ij')
    matcap = str(tmp_path / "matcap.png")
    save_u8(matcap, np.stack([xs * 4, ys * 5, 255 - xs * 3], -1).clip(0, 255).astype(np.uint8))
    r = OfflineRenderer(render_res=(32, 32), shading_mode=mode, matcap_path=matcap, device=DEV)
    assert not hasattr(pipe.tracer, "fused_normals")
    rb = r.render_lookat(pipe, f=[1.2, 0.9, 1.5], t=[0, 0, 0], fov=40.0, device=DEV)
    assert not hasattr(pipe.tracer, "fused_normals")          # set for the render only
    # hit mask and depth are the plain tracer's (fused_normals off) on the same rays
    from wisp.core import Rays
    from wisp.trainers.tracker.offline_renderer import _look_at
    o, d = _look_at([1.2, 0.9, 1.5], [0, 0, 0], 32, 32, fov=40.0, device=DEV)
    with torch.no_grad():
        plain = pipe.tracer(pipe.nef, rays=Rays(o, d, dist_min=0, dist_max=5)).reshape(32, 32, -1)
    assert torch.equal(rb.hit, plain.hit) and torch.equal(rb.depth, plain.depth) and torch.equal(rb.xyz, plain.xyz)
    # in batches of 300 rays (the last one short): the plain tracer's packs laid end to end.  (Not the unbatched picture bit for
    # bit: the marching step's nugget search of the LAST ray of a call is bounded by the number of packs - the reference's
    # find_depth_bound quirk the step kernels reproduce - so a pack boundary can move single pixels.)
    batched = OfflineRenderer(render_res=(32, 32), render_batch=300, shading_mode=mode, matcap_path=matcap, device=DEV)
    pipe.tracer.fused_normals = False                         # a value of the user's own comes back too
    rbb = batched.render_lookat(pipe, f=[1.2, 0.9, 1.5], t=[0, 0, 0], fov=40.0, device=DEV)
    assert pipe.tracer.fused_normals is False
    del pipe.tracer.fused_normals
    with torch.no_grad():
        packs = [pipe.tracer(pipe.nef, rays=pk) for pk in Rays(o, d, dist_min=0, dist_max=5).split(300)]
    assert [int(pk.hit.shape[0]) for pk in packs] == [300, 300, 300, 124]
    assert torch.equal(rbb.hit.reshape(-1), torch.cat([pk.hit for pk in packs]))
    assert torch.equal(rbb.depth.reshape(-1), torch.cat([pk.depth for pk in packs]).reshape(-1))
    assert rbb.rgb.shape == (32, 32, 3) and bool(torch.isfinite(rbb.rgb).all()) and 0.0 <= float(rbb.rgb.min()) and float(rbb.rgb.max()) <= 1.0
    assert int((rbb.hit != rb.hit).sum()) <= 8                # at most the pack boundaries' neighbourhoods
    assert rb.rgb.shape == (32, 32, 3) and rb.hit.shape == (32, 32, 1) and rb.depth.shape == (32, 32, 1)
    assert bool(torch.isfinite(rb.rgb).all()) and float(rb.rgb.min()) >= 0.0 and float(rb.rgb.max()) <= 1.0
    assert 100 < int(rb.hit.sum()) < 1000
    if mode == "rb" and tex:                                  # colours of the field, not normal colours
        with torch.no_grad():
            want = pipe.nef(coords=rb.xyz[rb.hit[..., 0]], channels="rgb")
        assert float((rb.rgb[rb.hit[..., 0]] - want).abs().max()) <= 1e-5
    if mode == "normal":
        snap = r.render_snapshot(pipe, f=[1.2, 0.9, 1.5], t=[0, 0, 0], fov=40.0, aa=2, camera_clamp=[0, 5])
        assert snap.rgb.shape == (32, 32, 3) and not snap.rgb.is_cuda
        assert torch.allclose(snap.rgb, rb.rgb.cpu().permute(1, 0, 2), atol=1e-6)
        vis = r.sdf_slice(pipe.nef, dim=2)
        nrm = r.normal_slice(pipe.nef, dim=0)
        assert vis.shape == (32, 32, 3) and nrm.shape == (32, 32, 3) and np.isfinite(vis).all() and np.isfinite(nrm).all()
        assert (vis == np.array([1.0, 0.38, 0.0])).all(-1).any()           # the sphere's interior is on the slice


def test_train_nglod_script_end_to_end(tmp_path):
    """scripts/train_nglod.py on the procedural torus at a small level for a few epochs: the IoU rises and the PNGs exist"""
    out = tmp_path / "out"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "train_nglod.py"), "--write-test-mesh", str(tmp_path / "mesh"),
                        "--level", "5", "--num-lods", "3", "--num-samples", "4000", "--mesh-samples", "200000", "--epochs", "4",
                        "--size", "48", "48", "--out-dir", str(out)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    rec = json.loads(r.stdout.strip().splitlines()[-1])
    record("script", iou_before=rec["iou_before"], iou_after=rec["iou_after"], hits=rec["hits"], seconds=rec["seconds"])
    assert rec["iou_after"] > rec["iou_before"]
    for name in ("render", "slice_x", "slice_y", "slice_z"):
        assert os.path.getsize(rec[name]) > 100
    assert rec["hits"] > 50
