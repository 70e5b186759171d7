"""Child process of tests/test_gpu_hashgrid_exact.py::test_backward_under_environment_switches (not collected by pytest).

csrc/hashgrid.hip reads WISP_HG_BWD_MERGE, WISP_HG_BWD_BIN, WISP_HG_BWD_QUEUE, WISP_HG_STRIP_BUCKETS, WISP_HG_EMIT_SMALL_BELOW and
WISP_HG_EMIT_WIDE once per process, so a setting needs a fresh process: this one runs the backward case list of
tests/hashgrid_exact_ref.py under whatever the environment says, compares every table with the float64 reference bit for bit
(zero table and seeded table) and prints one JSON line per case.  Exit status 1 when a case differs.
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (HERE, ROOT, os.path.join(ROOT, "kaolin-wisp_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch                                    # noqa: E402

import hashgrid_exact_ref as R                  # noqa: E402

DEV = "cuda:0"


def main():
    import wisp._C as C
    bad = 0
    for name in R.BWD_NAMES:
        case = R.bwd_case(name)
        want = R.reference_backward(case)["grad"]
        td = R.DTYPES[case["dtype"]]
        coords, first = case["coords"].to(DEV), case["first_idx"].to(DEV)
        g = case["grad_out"].float().to(td).to(DEV)
        differ = []
        for seeded in (False, True):
            out = case["seeds"].float().to(DEV) if seeded else None
            got = C.hashgrid_interpolate_backward(coords, g, (case["rows"], case["F"]), first, case["res"], case["bitwidth"],
                                                  case["zero_from_col"], out=out)
            torch.cuda.synchronize()
            w = (want + (case["seeds"] if seeded else 0.0)).float()
            got = got.cpu()
            same = torch.equal(got, w) and torch.equal(got.abs().view(torch.int32), w.abs().view(torch.int32))
            if not same:
                at = torch.nonzero(got != w)
                differ.append(dict(seeded=seeded, count=int(at.shape[0]),
                                   first=[(tuple(b.tolist()), float(got[tuple(b)]), float(w[tuple(b)])) for b in at[:4]]))
        bad += bool(differ)
        print(json.dumps(dict(name=name, n=case["n"], levels=case["res"], ok=not differ, differ=differ)), flush=True)
        R._cases.pop(name)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
