"""GPU: the image application - wisp_image_sample and ImageDataset against the reference's recorded output and the torch
restatement, the fused whole-image render (wisp_image_field_render) against the CPU oracle composition and its own structural
identities, the chunked fallback, ImageTrainStep against torch.optim.Adam, and scripts/train_image.py end to end.

Measured on an MI355X (the run is recorded line by line in profiles/image_app_gpu_test_margins.jsonl), max error against the CPU
oracle: fresh field 6.0e-8 (hidden 64 and 128, bound 3e-6); after 300 training steps E_mod = 1.2e-7 / E_fused = 1.8e-7 at hidden 64
and 1.8e-7 / 1.8e-7 at hidden 128 (bound max(3e-6, 2 E_mod) = 3e-6); squared-error sum within 3.9e-8 relative of the float64 sum
(bound 4 * 2^-24 = 2.4e-7)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import image_ref
from gpu_helpers import DEV, _assert_same_adam_trajectory, margin, ohash, onerf, snapshot_first_grad

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _C():
    import wisp._C as C
    return C


def _field(hidden=64, num_lods=16, bitwidth=14, max_res=128, multiscale='cat', num_layers=1, seed=0, std=0.01):
    from wisp.models.grids import HashGrid
    from wisp.models.nefs import ImageNeuralField
    torch.manual_seed(seed)
    grid = HashGrid.from_geometric(None, feature_dim=2, num_lods=num_lods, multiscale_type=multiscale, feature_std=std,
                                   codebook_bitwidth=bitwidth, min_grid_res=16, max_grid_res=max_res)
    return ImageNeuralField(grid, hidden_dim=hidden, num_layers=num_layers).to(DEV)


def _oracle_rgb(nef, coords_cpu, hidden):
    """The CPU oracle composition of test_image_field_config_c1_fits_and_matches_oracle_2d over this field's parameters."""
    grid = nef.grid
    L = grid.num_lods
    feats = ohash.grid_interpolate(coords_cpu, L - 1, 'cat', 2, grid.resolutions, grid.codebook_bitwidth,
                                   grid.codebook.feats.detach().cpu(), grid.codebook.begin_idxes.cpu())
    dec = onerf.OracleDecoder(2 * L + 14, 3, hidden, 1, True)
    dec.load_state_dict({k: v.detach().cpu() for k, v in nef.decoder.state_dict().items()})
    with torch.no_grad():
        return torch.sigmoid(dec(torch.cat([feats, onerf.positional_embed(coords_cpu, 3, include_input=True)], -1)))


def _bank(h, w):
    return torch.from_numpy(image_ref.procedural_image(h, w)).to(DEV)


# ------------------------------------------------------------------------------------------------ 1. sampling
def test_image_sample_equals_the_reference_fixture(golden_dir):
    C = _C()
    fix = np.load(os.path.join(golden_dir, "image_dataset_ref.npz"))
    img = torch.from_numpy(fix["image"]).to(DEV)
    h, w = img.shape[:2]
    out = C.image_sample(img, torch.arange(h * w, device=DEV))
    assert np.array_equal(out["coords"].cpu().numpy(), fix["coords"]) and np.array_equal(out["rgb"].cpu().numpy(), fix["pixels"])
    g = torch.Generator().manual_seed(1)
    idx = torch.cat([torch.tensor([0, h * w - 1]), torch.randint(0, h * w, (500,), generator=g)])
    out = C.image_sample(img, idx.to(DEV))
    assert np.array_equal(out["coords"].cpu().numpy(), fix["coords"][idx.numpy()])
    assert np.array_equal(out["rgb"].cpu().numpy(), fix["pixels"][idx.numpy()])


@pytest.mark.parametrize("size", [(37, 23), (1, 5), (5, 1), (4097, 3), (800, 800)])
def test_image_sample_equals_the_torch_restatement(size):
    C = _C()
    h, w = size
    img = torch.from_numpy(image_ref.seeded_image(h, w, seed=h + w))
    g = torch.Generator().manual_seed(h)
    idx = torch.cat([torch.tensor([0, h * w - 1, -1]), torch.randint(0, h * w, (20000,), generator=g), torch.arange(min(h * w, 5000))])
    out = C.image_sample(img.to(DEV), idx.to(DEV))
    want_c, want_p = image_ref.torch_sample(img, idx)
    assert out["coords"].dtype == torch.float32 and out["coords"].shape == (idx.shape[0], 2) and out["rgb"].shape == (idx.shape[0], 3)
    assert torch.equal(out["coords"].cpu(), want_c) and torch.equal(out["rgb"].cpu(), want_p)
    only = C.image_sample(img.to(DEV), idx.to(DEV), want=("coords",))
    assert set(only) == {"coords"} and torch.equal(only["coords"], out["coords"])
    empty = C.image_sample(img.to(DEV), torch.zeros(0, dtype=torch.int64, device=DEV))
    assert empty["coords"].shape == (0, 2) and empty["rgb"].shape == (0, 3)


def test_image_dataset_items_are_device_tensors_of_the_sampled_indices(tmp_path):
    from wisp.datasets import ImageDataset
    img = image_ref.seeded_image(37, 23, seed=9)
    path = str(tmp_path / "img.png")
    image_ref.write_png(path, img)
    ds = ImageDataset(path, num_pixels_per_image=333, device=DEV)
    assert ds.image_u8.is_cuda and ds.image_u8.dtype == torch.uint8 and (ds.h, ds.w, len(ds)) == (37, 23, 100)
    torch.cuda.manual_seed(11)
    c, p = ds[5]
    assert c.is_cuda and p.is_cuda and c.shape == (333, 2) and p.shape == (333, 3)
    torch.cuda.manual_seed(11)
    idx = torch.randint(0, 37 * 23, (333,), device=DEV)
    c2, p2 = ds.sample(idx)
    assert torch.equal(c, c2) and torch.equal(p, p2)
    want_c, want_p = image_ref.torch_sample(torch.from_numpy(img), idx)
    assert torch.equal(c.cpu(), want_c) and torch.equal(p.cpu(), want_p)
    assert torch.equal(ds.coords[idx.cpu()], want_c) and torch.equal(ds.pixels[idx.cpu()], want_p)


# ------------------------------------------------------------------------------------------------ 2. fused render vs oracle
@pytest.mark.parametrize("hidden", [64, 128])
def test_fused_render_matches_the_oracle_on_a_fresh_field(hidden):
    from wisp.models.nefs import fused_render_shape
    nef = _field(hidden)
    assert fused_render_shape(nef) is not None and nef.input_dim == 46
    H = 64
    coords = _C().image_sample(None, torch.arange(H * H, device=DEV), want=("coords",), size=(H, H))["coords"]
    want = _oracle_rgb(nef, coords.cpu(), hidden)
    got = nef.render_image(H, H)
    err = float((got.cpu() - want).abs().max())
    margin(f"fused render vs oracle, fresh field, hidden {hidden}", err, 3e-6)


@pytest.mark.parametrize("hidden", [64, 128])
def test_fused_render_matches_the_oracle_after_training(hidden):
    """300 ImageTrainStep steps on a procedural 64 x 64 image, then the fused render and the modular nef.rgb against the CPU oracle:
    both are fp32 evaluations of one expression in different summation orders, so the fused error may be at most twice the
    modular one (or the fresh-field bound 3e-6)."""
    from wisp.trainers import ImageTrainStep
    nef = _field(hidden)
    H = 64
    bank = _bank(H, H)
    step = ImageTrainStep(nef, lr=1e-3, eps=1e-15, grid_lr_weight=50.0)
    g = torch.Generator(device=DEV).manual_seed(3)
    first = last = None
    for it in range(300):
        idx = torch.randint(0, H * H, (2048,), device=DEV, generator=g)
        s = _C().image_sample(bank, idx)
        last = float(step.step(s["coords"], s["rgb"]))
        first = last if first is None else first
    assert last < 0.5 * first, (first, last)
    coords = _C().image_sample(None, torch.arange(H * H, device=DEV), want=("coords",), size=(H, H))["coords"]
    want = _oracle_rgb(nef, coords.cpu(), hidden)
    with torch.no_grad():
        e_mod = float((nef.rgb(coords).cpu() - want).abs().max())
    e_fused = float((nef.render_image(H, H).cpu() - want).abs().max())
    print(f"hidden {hidden}: E_mod = {e_mod:.3e}, E_fused = {e_fused:.3e}")
    margin(f"modular render vs oracle, trained, hidden {hidden} (E_mod, informative)", e_mod, float("inf"))
    margin(f"fused render vs oracle, trained, hidden {hidden}", e_fused, max(3e-6, 2 * e_mod))


# ------------------------------------------------------------------------------------------------ 3. structural identities
@pytest.mark.parametrize("hidden,size", [(64, (37, 23)), (128, (200, 301)), (40, (64, 64))])
def test_fused_render_structural_identities(hidden, size):
    C = _C()
    nef = _field(hidden, seed=2, std=0.3)
    with torch.no_grad():
        for p in nef.decoder.parameters():
            p.mul_(3.0)                                         # colours spread over (0, 1), relu masks exercised
    h, w = size
    n = h * w
    bank = torch.from_numpy(image_ref.seeded_image(h, w, seed=4)).to(DEV)
    whole = nef.render_image(h, w)
    assert whole.shape == (n, 3) and whole.dtype == torch.float32 and float(whole.min()) > 0 and float(whole.max()) < 1
    assert float(whole.max() - whole.min()) > 0.2
    # any split into ranges
    g = torch.Generator().manual_seed(7)
    cuts = sorted(set([0, n] + torch.randint(0, n, (6,), generator=g).tolist() + [1, 255, 256, 257]))
    cuts = [c for c in cuts if c <= n]
    parts = torch.cat([nef.render_image(h, w, first=a, count=b - a) for a, b in zip(cuts[:-1], cuts[1:])])
    assert torch.equal(parts, whole)
    assert nef.render_image(h, w, first=5, count=0).shape == (0, 3)
    # explicit coordinates from the sampling kernel
    grid, l1, lout = nef.grid, nef.decoder.layers[0], nef.decoder.lout
    packed, hp = C.image_field_pack_weights(l1.weight, l1.bias, lout.weight, lout.bias, grid.num_lods)
    args = (grid.codebook.feats.detach(), grid.codebook.begin_idxes, grid.codebook.resolutions.reshape(-1).tolist(), grid.codebook_bitwidth,
            grid.num_lods - 1, packed, hp)
    coords = C.image_sample(bank, torch.arange(n, device=DEV), want=("coords",))["coords"]
    by_coords, _, _ = C.image_field_render(h, w, 0, n, *args, coords=coords)
    assert torch.equal(by_coords, whole)
    # an explicit LOD: the default is the last one; another one is what rgb() computes for it (both sides are within 3e-6 of the
    # exact value, the bound of the oracle tests, hence 6e-6 between them); values rgb() has no levels for are refused
    assert torch.equal(nef.render_image(h, w, lod=grid.num_lods - 1), whole)
    with torch.no_grad():
        modular = nef.rgb(coords, 5)
    low = nef.render_image(h, w, lod=5)
    assert not torch.equal(low, whole)
    margin(f"fused render at lod 5 vs nef.rgb, hidden {hidden}", float((low - modular).abs().max()), 6e-6)
    for bad in (-1, grid.num_lods + 1):
        with pytest.raises(ValueError):
            nef.render_image(h, w, lod=bad)
    # u8 output, alone and together with the others
    u8 = nef.render_image(h, w, out='u8')
    assert u8.dtype == torch.uint8 and torch.equal(u8, (whole * 255).byte())
    f32_b, u8_b, part_b = C.image_field_render(h, w, 0, n, *args, gts_u8=bank, want_f32=True, want_u8=True, want_err=True)
    assert torch.equal(f32_b, whole) and torch.equal(u8_b, u8)
    # two launches: identical bytes, error partials included
    f32_c, u8_c, part_c = C.image_field_render(h, w, 0, n, *args, gts_u8=bank, want_f32=True, want_u8=True, want_err=True)
    assert torch.equal(f32_c, f32_b) and torch.equal(u8_c, u8_b)
    assert part_b.dtype == torch.float64 and part_b.shape[0] == -(-n // 256) and torch.equal(part_b.view(torch.int64), part_c.view(torch.int64))
    _, _, only_err = C.image_field_render(h, w, 0, n, *args, gts_u8=bank, want_f32=False, want_err=True)
    assert torch.equal(only_err.view(torch.int64), part_b.view(torch.int64))
    # the squared-error sum: three fp32 roundings per term (the difference, the conversion's division, the square) plus slack
    want = ((whole.double() - bank.reshape(-1, 3).double() / 255.0) ** 2).sum()
    got = part_b.sum()
    rel = abs(float(got) - float(want)) / float(want)
    margin(f"squared-error sum, hidden {hidden}, {h}x{w}", rel, 4 * 2.0 ** -24)
    _, err = nef.render_image(h, w, out='u8', gts_u8=bank)
    assert float(err) == float(got)


# ------------------------------------------------------------------------------------------------ 4. fallback
@pytest.mark.parametrize("case", ["sum", "two_layers", "hidden256", "disabled"])
def test_other_field_shapes_fall_back_to_chunked_rgb(case, monkeypatch):
    from wisp.models.nefs import fused_render_shape
    nef = {"sum": lambda: _field(multiscale='sum'), "two_layers": lambda: _field(num_layers=2), "hidden256": lambda: _field(hidden=256),
           "disabled": lambda: _field()}[case]()
    if case == "disabled":
        monkeypatch.setenv("WISP_IMAGE_RENDER_FUSED", "0")
    assert fused_render_shape(nef) is None
    h, w = 45, 31
    bank = torch.from_numpy(image_ref.seeded_image(h, w, seed=4)).to(DEV)
    coords = _C().image_sample(bank, torch.arange(h * w, device=DEV), want=("coords",))["coords"]
    with torch.no_grad():
        want = torch.cat([nef.rgb(c) for c in torch.split(coords, 400)])
    got = nef.render_image(h, w, chunk=400)
    assert torch.equal(got, want)
    assert torch.equal(nef.render_image(h, w, first=100, count=700, chunk=400), torch.cat([nef.rgb(coords[100:500]), nef.rgb(coords[500:800])]).detach())
    u8, err = nef.render_image(h, w, out='u8', gts_u8=bank, chunk=400)
    assert torch.equal(u8, (want * 255).byte())
    ref = ((want - bank.reshape(-1, 3) / 255.0) ** 2).double().sum()
    assert abs(float(err) - float(ref)) <= 1e-12 * float(ref)


# ------------------------------------------------------------------------------------------------ 5. the training step
def test_image_train_step_matches_torch_adam():
    """ImageTrainStep (mean squared error, Adam over the flat buffer in one fused launch) against the same field stepped with
    torch.optim.Adam, as test_sdf_train_step_matches_torch_adam does it; then the captured graph against the eager step, and lr."""
    import copy
    from wisp.trainers import ImageTrainStep
    nef = _field(64, seed=5, std=0.05)
    ref = copy.deepcopy(nef)
    groups = [{"params": [p for n, p in ref.named_parameters() if 'decoder' in n], "lr": 1e-3},
              {"params": [p for n, p in ref.named_parameters() if 'decoder' not in n and 'grid' in n], "lr": 2e-3},
              {"params": [p for n, p in ref.named_parameters() if 'decoder' not in n and 'grid' not in n], "lr": 1e-3}]
    opt = torch.optim.Adam([g for g in groups if g["params"]], eps=1e-15)
    tr = ImageTrainStep(nef, lr=1e-3, eps=1e-15, grid_lr_weight=2.0)
    H = 64
    bank = _bank(H, H)
    g = torch.Generator(device=DEV).manual_seed(1)
    batches = []
    for _ in range(8):
        s = _C().image_sample(bank, torch.randint(0, H * H, (512,), device=DEV, generator=g))
        batches.append((s["coords"], s["rgb"]))
    grads = []
    snapshot_first_grad(tr, grads)
    for it in range(4):
        xy, rgb = batches[it]
        l1 = tr.step(xy, rgb)
        opt.zero_grad()
        l2 = torch.nn.functional.mse_loss(ref.rgb(xy), rgb)
        l2.backward()
        if it == 0:
            flat = grads[0]
            for (n1, p1), (n2, p2) in zip(nef.named_parameters(), ref.named_parameters()):
                if not p1.requires_grad:                        # the embedder's frequency bands: a constant on both sides
                    assert p2.grad is None and torch.equal(p1, p2)
                    continue
                off = (p1.grad.data_ptr() - tr.flat.grad.data_ptr()) // 4
                g1 = flat[off:off + p1.numel()].view_as(p1)
                sc = max(float(p2.grad.abs().max()), 1e-12)
                margin(f"image step grad {n1}", float((g1 - p2.grad).abs().max()), 1e-4 * sc)
        opt.step()
        assert abs(float(l1) - float(l2)) <= 1e-5 * max(1.0, abs(float(l2)))
    for (n1, p1), (n2, p2) in zip(sorted(nef.named_parameters()), sorted(ref.named_parameters())):
        _assert_same_adam_trajectory(p1, p2, n1, steps=4, max_lr=2e-3)

    # captured graph == eager, on the same batches from the same state
    eager, graphed = _field(64, seed=6, std=0.05), _field(64, seed=6, std=0.05)
    te = ImageTrainStep(eager, lr=1e-3, eps=1e-15, grid_lr_weight=2.0)
    tg = ImageTrainStep(graphed, lr=1e-3, eps=1e-15, grid_lr_weight=2.0).capture(512)
    assert tg.static_inputs()[0].shape == (512, 2)
    for it, (xy, rgb) in enumerate(batches):                      # (same kernels, same arguments; only float atomics of the table
        le, lg = te.step(xy, rgb), tg.step(xy, rgb)              #  gradient may add in another order: the bound of the SDF step's test)
        assert abs(float(le) - float(lg)) <= 1e-6 * max(1.0, abs(float(le))), it
        if it == 0:
            assert float(le) == float(lg)                         # a forward pass from identical parameters: the same bits
    for (n1, p1), (n2, p2) in zip(sorted(eager.named_parameters()), sorted(graphed.named_parameters())):
        _assert_same_adam_trajectory(p1, p2, "graph " + n1, steps=len(batches), max_lr=2e-3)

    # lr is read at every step
    a, b = _field(64, seed=7, std=0.05), _field(64, seed=7, std=0.05)
    ta, tb = ImageTrainStep(a, lr=1e-3, eps=1e-15), ImageTrainStep(b, lr=1e-3, eps=1e-15)
    ta.step(*batches[0]); tb.step(*batches[0])
    before_a, before_b = ta.flat.data.clone(), tb.flat.data.clone()
    tb.lr = 1e-5
    ta.step(*batches[1]); tb.step(*batches[1])
    moved_a, moved_b = float((ta.flat.data - before_a).abs().max()), float((tb.flat.data - before_b).abs().max())
    assert moved_b < 0.05 * moved_a and moved_b > 0, (moved_a, moved_b)


# ------------------------------------------------------------------------------------------------ 6. end to end
@pytest.mark.parametrize("fused_step", [False, True])
def test_train_image_script_end_to_end(tmp_path, fused_step):
    from wisp.ops.image import load_u8
    img_path, log_dir = str(tmp_path / "test.png"), str(tmp_path / "run")
    cmd = [sys.executable, os.path.join(ROOT, "scripts", "train_image.py"), "--write-test-image", img_path, "--size", "256", "256",
           "--epochs", "10", "--log-dir", log_dir] + (["--fused-step"] if fused_step else [])
    run = subprocess.run(cmd, capture_output=True, text=True, timeout=420)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-4000:]
    rec = json.loads(run.stdout.strip().splitlines()[-1])
    print(rec)
    assert rec["step"] == ("ImageTrainStep" if fused_step else "ImageTrainer") and (rec["h"], rec["w"]) == (256, 256)
    assert np.isfinite(rec["psnr"]) and rec["psnr"] > rec["psnr_first_epoch"], rec
    pred, gts = load_u8(os.path.join(log_dir, "img_pred.png")), load_u8(os.path.join(log_dir, "img_gts.png"))
    assert pred.shape == (256, 256, 3) and np.array_equal(gts, load_u8(img_path))
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    try:
        import train_image
        assert np.array_equal(gts, train_image.procedural_image(256, 256))
    finally:
        sys.path.pop(0)
