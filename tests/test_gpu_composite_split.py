"""wisp_composite_loss with long rays split over the four waves of their workgroup (composite_loss_split_kernel, render.hip)
against the one-wave-per-ray kernel it replaces (WISP_COMPOSITE_SPLIT=0) and against the three separate launches."""
import numpy as np
import pytest
import torch

from gpu_helpers import cuda, _C

pytestmark = pytest.mark.gpu

BG = (0.2, 0.5, 0.9)
# four consecutive rays share a workgroup, one per wave
LENS = [0, 1, 63, 64,
        65, 127, 128, 129,             # all four long
        191, 192, 193, 255,
        256, 257, 718, 2047,
        0, 0, 0, 2048,                 # the long ray on wave 3, nothing on waves 0-2
        2049, 4000, 5, 300,            # more than the split path holds: three passes on their own wave
        1024, 1025, 0, 70,             # the longest ray the split path takes, and the first it does not
        40, 500, 64, 900,
        10, 0, 1100, 33,
        1500, 700, 1300, 3,
        600]                           # R % 4 == 1: the last workgroup has one ray, a long one, and three waves without a ray
ZERO_RAY, DENSE_RAY = 14, 19           # the 718-sample ray gets density 0 everywhere, the 2048-sample ray underflows T


def _batch(lens, seed):
    rng = np.random.default_rng(seed)
    offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    S, R = int(offs[-1]), len(lens)
    color = rng.uniform(0, 1, (S, 3)).astype(np.float32)
    dens = (rng.uniform(0, 30, (S, 1)) * (rng.uniform(size=(S, 1)) < 0.6)).astype(np.float32)     # zeros: tau = 0
    delt = rng.uniform(1e-3, 4e-2, (S, 1)).astype(np.float32)
    gts = rng.uniform(-1.5, 2.5, (R, 3)).astype(np.float32)              # |rgb - gt| on both sides of the huber knee
    return offs, color, dens, delt, gts


@pytest.fixture(scope="module")
def batch():
    assert len(LENS) % 4 == 1 and LENS[-1] > 64 and LENS[ZERO_RAY] == 718 and LENS[DENSE_RAY] == 2048
    offs, color, dens, delt, gts = _batch(LENS, 911)
    dens[offs[ZERO_RAY]:offs[ZERO_RAY + 1]] = 0.0
    dens[offs[DENSE_RAY]:offs[DENSE_RAY + 1]] = 30.0
    delt[offs[DENSE_RAY]:offs[DENSE_RAY + 1]] = 0.04
    tau = (dens * delt).astype(np.float64)[offs[DENSE_RAY]:offs[DENSE_RAY + 1]]
    assert np.float32(np.exp(-tau.sum())) == 0.0                        # T underflows along that ray
    return dict(R=len(LENS), offs=offs, t=[cuda(x) for x in (color, dens, delt, offs, gts)])


def _run(monkeypatch, split, t, R, kind):
    if split is None:
        monkeypatch.delenv("WISP_COMPOSITE_SPLIT", raising=False)
    else:
        monkeypatch.setenv("WISP_COMPOSITE_SPLIT", split)
    c, d, dl, o, g = t
    return _C().composite_loss(c, d, dl, o, R, BG, g, kind, with_rgb=True)


def _compare(name, got, want):
    """loss, grad_color and rgb bit for bit; grad_density equal or within the bound of
    test_composite_loss_in_one_launch_equals_the_three_launches (rtol 2e-6, atol 1e-6 max|.|).  Observed on an MI355X: a maximum
    difference of 0 in every case of this file - the split kernel writes its product-sums out as the one-wave kernel rounds them."""
    assert torch.equal(got[3], want[3]), name + ": rgb"
    assert torch.equal(got[1], want[1]), name + ": grad_color"
    assert torch.equal(got[0], want[0]), name + ": loss"
    diff = float((got[2] - want[2]).abs().max())
    print(f"{name}: max |grad_density difference| = {diff:.3e} (max |grad_density| = {float(want[2].abs().max()):.3e})")
    torch.testing.assert_close(got[2], want[2], rtol=2e-6, atol=1e-6 * float(want[2].abs().max()))


@pytest.mark.parametrize("kind", ["huber", "l2", "l1"])
def test_split_equals_one_wave_per_ray(batch, kind, monkeypatch):
    R, t = batch["R"], batch["t"]
    off = _run(monkeypatch, "0", t, R, kind)
    assert float(off[2].abs().max()) > 0 and np.isfinite(float(off[0]))
    for split in (None, "1"):
        on = _run(monkeypatch, split, t, R, kind)
        _compare(f"{kind} split={split}", on, off)
        for _ in range(3):                                              # same bits from call to call
            again = _run(monkeypatch, split, t, R, kind)
            assert all(torch.equal(a, b) for a, b in zip(again, on))
    # the three separate launches: colours and their gradient bit for bit, the density gradient within that test's tolerance
    C = _C()
    c, d, dl, o, g = t
    rgb = C.composite_fwd(c, d, dl, None, None, o, R, BG)[0]
    loss3, g_rgb = C.rgb_loss(rgb, g, kind)
    gc3, gd3 = C.composite_bwd(g_rgb, None, None, c, d, dl, None, None, o, BG)
    on = _run(monkeypatch, None, t, R, kind)
    assert torch.equal(on[3], rgb) and torch.equal(on[1], gc3)
    torch.testing.assert_close(on[2], gd3, rtol=2e-6, atol=1e-6 * float(gd3.abs().max()))
    assert abs(float(on[0]) - float(loss3)) <= 2e-6 * abs(float(loss3))


@pytest.mark.parametrize("kind", ["huber", "l2", "l1"])
def test_split_less_than_one_workgroup(kind, monkeypatch):
    """R = 3: one workgroup, its fourth wave without a ray, one long ray."""
    lens = [7, 333, 0]
    offs, color, dens, delt, gts = _batch(lens, 912)
    t = [cuda(x) for x in (color, dens, delt, offs, gts)]
    off = _run(monkeypatch, "0", t, 3, kind)
    for split in (None, "1"):
        _compare(f"{kind} R=3 split={split}", _run(monkeypatch, split, t, 3, kind), off)
