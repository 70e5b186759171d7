"""Device side of tests/test_gpu_composite_exact.py, and the child process of its test_loss_under_wave_counts (not collected by pytest).

The helpers call the C entry points of csrc/render.hip directly (marshalling as in wisp/_C.py) so that every output lies in front of
guard values and every input in front of extra rows; `Guards.check` looks at all of them after a call.

As a program: wisp_composite_loss reads WISP_COMPOSITE_WAVES once per process, so a setting needs a fresh process.  This one runs the
composite_loss case list of tests/composite_exact_ref.py (Family A: bit for bit; Family B: the worst error in units of the per-element
bound) under whatever the environment says and prints one JSON line per case.  Exit status 1 when a Family A case differs.
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (HERE, ROOT, os.path.join(ROOT, "kaolin-wisp_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np                              # noqa: E402
import torch                                    # noqa: E402

import composite_exact_ref as R                 # noqa: E402

DEV = "cuda:0"
GUARD = 64                                      # elements behind an output, rows behind an input
SENTINEL = 7777.0
LOSS_KIND = {"huber": 0, "l2": 1, "l1": 2}


def _C():
    import wisp._C as C
    return C


class Guards:
    """device buffers with guard values behind them: outputs are pre-filled with the sentinel as well, so an element a kernel
    skips shows up in the comparison"""

    def __init__(self):
        self.items = []

    def inp(self, a, dtype=torch.float32, pad=-SENTINEL, what="input"):
        t = torch.as_tensor(np.asarray(a)).to(dtype)
        tail = torch.full((GUARD,) + tuple(t.shape[1:]), pad, dtype=dtype)
        full = torch.cat([t, tail]).to(DEV)
        self.items.append((full, t.shape[0], tail, what))
        return full[:t.shape[0]]

    def out(self, shape, dtype=torch.float32, what="output"):
        n = int(np.prod(shape))
        fill = SENTINEL if dtype.is_floating_point else 0x5A
        full = torch.full((n + GUARD,), fill, dtype=dtype, device=DEV)
        self.items.append((full, n, torch.full((GUARD,), fill, dtype=dtype), what))
        return full[:n].view(shape)

    def check(self, call, keep=None):
        """after a call: every guard intact; then forget the outputs (the inputs, the first `keep` items, stay)"""
        torch.cuda.synchronize()
        for full, n, tail, what in self.items:
            assert torch.equal(full[n:].cpu(), tail), f"{call}: the values behind {what} were overwritten"
        if keep is not None:
            del self.items[keep:]


def _p(t):
    return _C()._p(t)


def composite_fwd(G, color, density, deltas, depths, ridx, starts, num_rays, bg):
    C = _C()
    S = color.shape[0]
    out = dict(rgb=G.out((num_rays, 3), what="rgb"), alpha=G.out((num_rays, 1), what="alpha"),
               depth=None if depths is None else G.out((num_rays, 1), what="depth"), hit=G.out((num_rays,), torch.uint8, what="hit"),
               weights=G.out((S, 1), what="weights"))
    _keep, bg_ptr = C._host_f32(bg)
    num_packs = num_rays if ridx is None else starts.shape[0]
    C._check(C.lib.wisp_composite_fwd(_p(color), _p(density), _p(deltas), _p(depths), _p(ridx), _p(starts), num_packs, S, num_rays, bg_ptr,
                                      _p(out["rgb"]), _p(out["alpha"]), _p(out["depth"]), _p(out["hit"]), _p(out["weights"]), C._stream()),
             "composite_fwd")
    out["hit"] = out["hit"].bool()
    return out


def composite_bwd(G, g_rgb, g_alpha, g_depth, color, density, deltas, depths, ridx, starts, bg):
    C = _C()
    S = color.shape[0]
    out = dict(grad_color=G.out((S, 3), what="grad_color"), grad_density=G.out((S, 1), what="grad_density"))
    _keep, bg_ptr = C._host_f32(bg)
    num_packs = starts.shape[0] - 1 if ridx is None else starts.shape[0]
    C._check(C.lib.wisp_composite_bwd(_p(g_rgb), _p(g_alpha), _p(g_depth), _p(color), _p(density), _p(deltas), _p(depths), _p(ridx), _p(starts),
                                      num_packs, S, bg_ptr, _p(out["grad_color"]), _p(out["grad_density"]), C._stream()), "composite_bwd")
    return out


def composite_loss(G, color, density, deltas, offsets, num_rays, bg, gt, kind, with_rgb=True, cells=None):
    """wisp_composite_loss with a workspace of `cells` partial sums (default: one per ray, what wisp._C.composite_loss guarantees
    at least; fewer: the grid-stride walk of composite_loss_kernel)"""
    C = _C()
    S = color.shape[0]
    cells = num_rays if cells is None else cells
    out = dict(loss=G.out((1,), what="loss"), grad_color=G.out((S, 3), what="grad_color"), grad_density=G.out((S, 1), what="grad_density"),
               rgb=G.out((num_rays, 3), what="rgb") if with_rgb else None)
    ws = G.out((cells,), what="the last partial-sum cell")
    _keep, bg_ptr = C._host_f32(bg)
    C._check(C.lib.wisp_composite_loss(_p(color), _p(density), _p(deltas), _p(offsets), num_rays, S, bg_ptr, _p(gt), LOSS_KIND[kind],
                                       _p(out["grad_color"]), _p(out["grad_density"]), _p(out["rgb"]), _p(out["loss"]), _p(ws), cells,
                                       C._stream()), "composite_loss")
    return out


def loss_inputs(G, c):
    """device inputs of wisp_composite_loss for a case of either family"""
    S = c["S"]
    return dict(color=G.inp(c["color"], what="color"), density=G.inp(np.reshape(c["density"], (S, 1)), what="density"),
                deltas=G.inp(np.reshape(c["delta"], (S, 1)), what="deltas"), offsets=G.inp(c["offs"], torch.int64, pad=S, what="offsets"),
                gt=G.inp(c["gt"], what="gt"))


def run_loss(G, d, c, kind, with_rgb=True, cells=None, keep=5):
    out = composite_loss(G, d["color"], d["density"], d["deltas"], d["offsets"], c["R"], c["bg"], d["gt"], kind, with_rgb, cells)
    G.check(f"composite_loss {c['name']} {kind}", keep=keep)
    return out


def differences(got, want, names):
    """[(name, count, first mismatches)] of the outputs that are not equal bit for bit"""
    bad = []
    for n in names:
        g, w = got[n].detach().cpu(), want[n]
        assert g.shape == w.shape and g.dtype == w.dtype, (n, g.shape, w.shape, g.dtype, w.dtype)
        if not torch.equal(g, w):
            at = torch.nonzero(g != w)
            bad.append((n, int(at.shape[0]), [(tuple(b.tolist()), float(g[tuple(b)]), float(w[tuple(b)])) for b in at[:4]]))
    return bad


def ratios(got, ref, scale, names):
    """worst |got - ref| / (2^-24 scale) per output; an error where the scale is 0 counts as infinite, one of at most TINY as none"""
    out = {}
    for n in names:
        err = np.abs(got[n].detach().cpu().double().numpy().reshape(ref[n].shape) - ref[n])
        err = np.where(err <= R.TINY, 0.0, err)
        unit = R.F32_EPS * scale[n]
        with np.errstate(divide="ignore", invalid="ignore"):
            q = np.where(err == 0, 0.0, err / unit)
        out[n] = float(q.max()) if q.size else 0.0
    return out


LOSS_OUT = ("loss", "grad_color", "grad_density", "rgb")
B_LOSS_OUT = ("grad_color", "grad_density", "rgb")


def main():
    bad = 0
    for name in R.WORKER_LOSS_NAMES:
        c = R.loss_case(name)
        G = Guards()
        d = loss_inputs(G, c)
        for kind in R.KINDS:
            diff = differences(run_loss(G, d, c, kind), R.reference_loss(c, kind), LOSS_OUT)
            bad += bool(diff)
            print(json.dumps(dict(family="A", name=name, kind=kind, rays=c["R"], ok=not diff, differ=diff)), flush=True)
    for name in ("main", "tail2", "three"):
        c = R.b_case(name)
        G = Guards()
        d = loss_inputs(G, c)
        for kind in R.KINDS:
            ref, scale, scale_e = R.reference_b_loss(c, kind)
            got = run_loss(G, d, c, kind)
            print(json.dumps(dict(family="B", name=name, kind=kind, rays=c["R"], ratios=ratios(got, ref, scale, B_LOSS_OUT),
                                  ratios_e=ratios(got, ref, scale_e, B_LOSS_OUT))), flush=True)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
