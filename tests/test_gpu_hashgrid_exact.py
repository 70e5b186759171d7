"""Exact-arithmetic tests of the hash-grid lookup, its backward, grad_coords and the corner query's backward
(csrc/hashgrid.hip, csrc/hashgrid_dev.h).

The inputs of tests/hashgrid_exact_ref.py make every product and every partial sum exactly representable, so every element a
kernel writes must equal the plain float64 reference BIT FOR BIT whatever the run merge, the buckets, the slots, the record form,
the emitter or flush width, the binary point of the fixed-point accumulators or the order of the fallbacks' float atomics:
`torch.equal` throughout, no tolerance anywhere in this file.  A bitwise mismatch on exact inputs is a defect of the kernel
(tests/test_hashgrid_exact_host.py rules out the reference and shows which paths each case reaches); the assertion message names
row and feature of the first mismatches.  Every backward is compared over the WHOLE table, untouched rows included, once into a
fresh zero table and once into a seeded integer `out`.
"""
import json
import os
import subprocess
import sys

import pytest
import torch

import hashgrid_exact_ref as R
from gpu_helpers import DEV, _C

pytestmark = pytest.mark.gpu

GUARD = 64                       # elements behind (and in front of) a buffer that a kernel must leave alone
_cache = {}


@pytest.fixture(scope="module", autouse=True)
def _release_cases():
    """cases, references and device inputs are shared by the tests of this file and freed when it finishes"""
    yield
    _cache.clear()
    R._cases.clear()
    _C()._slot_fits.clear()


def _dev(case):
    td = R.DTYPES[case["dtype"]]
    return dict(coords=case["coords"].to(DEV), grad_out=case["grad_out"].float().to(td).to(DEV), first_idx=case["first_idx"].to(DEV),
                table=case["table"].float().to(td).to(DEV))


def _describe(case):
    print(f"{case['name']}: n = {case['n']}, {case['dim']}-D, F = {case['F']}, {case['dtype']}, bitwidth {case['bitwidth']}, "
          f"levels {case['res']}, first_idx {case['first_idx'].tolist()}, zero_from_col {case['zero_from_col']}")


def _bwd(name_or_case):
    """(case, float64 reference gradient, device inputs), built once"""
    case = R.bwd_case(name_or_case) if isinstance(name_or_case, str) else name_or_case
    key = ("bwd", case["name"])
    if key not in _cache:
        _cache[key] = (case, R.reference_backward(case)["grad"], _dev(case))
    _describe(case)
    return _cache[key]


def _same(got, want, what):
    """bit for bit, compared on the host - with the bit patterns of the magnitudes as well: an equality that flushed denormals
    would not do"""
    got, want = got.detach().cpu(), want.detach().cpu()
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    if got.dtype == torch.float32:
        bits = lambda t: t.abs().view(torch.int32)
    else:
        bits = lambda t: t.abs().view(torch.int16)
    if torch.equal(got, want) and torch.equal(bits(got), bits(want)):
        return
    bad = torch.nonzero((got != want) | (bits(got) != bits(want)))
    first = [(tuple(b.tolist()), float(got[tuple(b)]), float(want[tuple(b)])) for b in bad[:6]]
    raise AssertionError(f"{what}: {bad.shape[0]} of {got.numel()} elements differ; ((row, column), got, want): {first}")


def _run_bwd(case, dev, out=None):
    got = _C().hashgrid_interpolate_backward(dev["coords"], dev["grad_out"], (case["rows"], case["F"]), dev["first_idx"], case["res"],
                                             case["bitwidth"], case["zero_from_col"], out=out)
    torch.cuda.synchronize()
    return got


def _check_bwd(case, want, dev, what=None, seeded=(False, True)):
    """into a fresh zero table and onto integer seeds; the whole table is compared"""
    what = what or case["name"]
    for s in seeded:
        if s and case["scale_exp"] != 0:
            continue                                         # (integer seeds plus a scaled gradient are no fp32 values)
        out = case["seeds"].float().to(DEV) if s else None
        got = _run_bwd(case, dev, out)
        _same(got, (want + (case["seeds"] if s else 0.0)).float(), f"{what} ({'seeded' if s else 'zero'} table)")
    return got


# ---------------------------------------------------------------------------------------------------- forward
def _fwd(case):
    key = ("fwd", case["name"], case["zero_from_col"], tuple(case["first_idx"].tolist()))
    if key not in _cache:
        _cache[key] = (R.reference_forward(case), _dev(case))
    _describe(case)
    return _cache[key]


def _run_fwd(case, dev, zero_from_col=None):
    got = _C().hashgrid_interpolate(dev["coords"], dev["table"], dev["first_idx"], case["res"], case["bitwidth"],
                                    case["zero_from_col"] if zero_from_col is None else zero_from_col)
    torch.cuda.synchronize()
    return got


@pytest.mark.parametrize("dim", [2, 3])
@pytest.mark.parametrize("dtype", R.FWD_DTYPES)
def test_forward_of_every_instantiation_equals_float64_reference(dtype, dim):
    """the 24 (dtype, F, dim) instantiations, each with 4 levels (output row a power of two: shifts) and 5 (divisions); every layout
    has a dense level below 258 (the 8-byte pair loads of one-dword rows) and hashed levels; W = F sizeof(T) / 4 runs through
    1, 2, 4 (buffer loads), 8 and 16 (the generic fetch; 16 with fewer waves per workgroup for the LDS staging)"""
    for F in R.FWD_F:
        for lods in (4, 5):
            case = R.fwd_case(dtype, F, dim, lods)
            want, dev = _fwd(case)
            _same(_run_fwd(case, dev), want, case["name"])


@pytest.mark.parametrize("W", sorted(R.FWD_WIDTHS))
def test_forward_writes_exactly_n_rows(W):
    """n = 1, 63, 64, 65 and 257 for one instantiation per row width: the output lies inside a larger seeded allocation, the rows
    are exact and the elements behind row n keep their seed"""
    C = _C()
    dtype, F = R.FWD_WIDTHS[W]
    td = R.DTYPES[dtype]
    for n in R.FWD_SMALL_N:
        case = R.fwd_case(dtype, F, 3, 5, n=n, claims=())
        want, dev = _fwd(case)
        width = case["L"] * F
        buf = torch.full((n * width + GUARD,), 7.0, dtype=td, device=DEV)
        _, res_arr, res_ptr = C._host_res(case["res"])
        C._check(C.lib.wisp_hashgrid_interpolate_fwd(C._p(dev["coords"]), n, 3, C._p(dev["table"]), C._DTYPE_CODE[td], F,
                                                     C._p(dev["first_idx"]), res_ptr, case["L"], case["bitwidth"], width, C._p(buf),
                                                     C._stream()), "hashgrid_interpolate_fwd")
        torch.cuda.synchronize()
        _same(buf[:n * width].view(n, width), want, case["name"])
        _same(buf[n * width:], torch.full((GUARD,), 7.0, dtype=td), f"{case['name']}: the elements behind row n")


@pytest.mark.parametrize("dim", [2, 3])
@pytest.mark.parametrize("bitwidth", [1, 6])
@pytest.mark.parametrize("dtype", ["f16", "bf16"])
def test_forward_pair_loads_on_tiny_tables(dtype, bitwidth, dim):
    """16-bit F = 2 (one dword per row): tables of 2 and of 64 rows per level, so that several corners of a sample share a row and
    a hashed pair load serves entries i and i ^ 1 of cells with even and with odd x"""
    case = R.fwd_tiny_case(dtype, bitwidth, dim)
    want, dev = _fwd(case)
    _same(_run_fwd(case, dev), want, case["name"])


@pytest.mark.parametrize("dtype,F", [("bf16", 2), ("f32", 2)])
def test_forward_with_a_padded_first_idx(dtype, F):
    """levels 1 and 2 start on odd rows (W = 1: 4-byte aligned pairs; W = 2: 8-byte rows)"""
    case = R.fwd_case(dtype, F, 3, 4, n=1000, pad=(0, 1, 2, 0), claims=("odd_start",))
    want, dev = _fwd(case)
    _same(_run_fwd(case, dev), want, case["name"])


@pytest.mark.parametrize("dtype,F", R.FWD_CUT)
def test_forward_zero_from_col(dtype, F):
    """cut after level 0, inside level 2 and at L F: the columns behind the cut are exactly zero"""
    for case in R.fwd_cut_cases(dtype, F):
        cut = case["zero_from_col"]
        want, dev = _fwd(case)
        got = _run_fwd(case, dev)
        _same(got, want, case["name"])
        assert int(got[:, cut:].count_nonzero()) == 0 and int(got[:, :cut].count_nonzero()) > 0


def test_forward_of_dense_2d_levels_and_their_spill_rows():
    """2-D, bitwidth 21: 256 / 512 / 1024 (no c = +1: the bound of res 256 is not dyadic) and 512 / 1024 / 512 with c = +1 on every
    axis - the +1 corner has index `res` and weight exactly 0; its read must hit the next level's row, or the table's last row on
    the last level, never leave the allocation"""
    for case in R.fwd_spill_cases():
        want, dev = _fwd(case)
        _same(_run_fwd(case, dev), want, case["name"])


# ---------------------------------------------------------------------------------------------------- backward
@pytest.mark.parametrize("name", R.BWD_NAMES)
def test_backward_equals_float64_reference(name):
    """both sides of every dispatch decision of launch_bwd (direct atomics / binned at 4095 / 4096; generic and compact queue
    emitter; merge refused for 3-D F = 8 and 16, kept for 2-D F = 8; bins refused for the emit LDS of 12 levels), sample counts
    around the emitter pieces, bucket geometries (strip-dealt dense buckets, a level below one bucket, one owner per bucket, coarse
    levels split over workgroups), odd level starts (8-byte flush), dead level suffixes and spill rows"""
    case, want, dev = _bwd(name)
    _check_bwd(case, want, dev)
    if "dead_levels" in case["claims"]:
        first_dead = -(-case["zero_from_col"] // case["F"])
        lo = int(case["first_idx"][first_dead])
        out = case["seeds"].float().to(DEV)
        got = _run_bwd(case, dev, out)
        _same(got[lo:], case["seeds"][lo:].float(), f"{name}: rows of the dead levels")


@pytest.mark.parametrize("name", ["generic f32 F2 n5000", "compact bf16 F2 3d n5000", "direct f32 F2 n4095"])
def test_backward_into_a_view_one_float_into_a_buffer(name):
    """`out` starts 4 bytes into a larger buffer (the flush's scalar path); the guard floats around it are unchanged"""
    case, want, dev = _bwd(name)
    numel = case["rows"] * case["F"]
    buf = torch.full((1 + numel + GUARD,), 9.0, dtype=torch.float32, device=DEV)
    out = buf[1:1 + numel].view(case["rows"], case["F"])
    out.copy_(case["seeds"].float())
    assert out.is_contiguous() and out.data_ptr() % 8 == 4
    got = _run_bwd(case, dev, out)
    assert got.data_ptr() == out.data_ptr()
    _same(got, (want + case["seeds"]).float(), f"{name} (view)")
    _same(torch.cat([buf[:1], buf[1 + numel:]]), torch.full((1 + GUARD,), 9.0), f"{name}: guard floats")


@pytest.mark.parametrize("name", R.ORDER_NAMES)
def test_backward_is_order_free(name):
    """the run order, a random permutation and the round-robin deal (nothing merges) of one multiset of samples give bit-identical
    tables, all equal to the reference"""
    case, want, dev = _bwd(name)
    tables = [_check_bwd(case, want, dev, seeded=(False,))]
    for order in ("perm", "alt"):
        other = R.reordered(case, order)
        tables.append(_check_bwd(other, want, _dev(other), seeded=(False,)))
    assert torch.equal(tables[0], tables[1]) and torch.equal(tables[0], tables[2])


@pytest.mark.parametrize("name", R.ORDER_NAMES)
def test_backward_slot_overflow_is_exact(name, monkeypatch):
    """Record slots forced to 2 % of their size and the no-merge order: slots fill (asserted through the slot statistics), the
    overflow goes through float atomics, and the gradient is still exact.  The run order with unscaled slots fills none."""
    C = _C()
    monkeypatch.setattr(C._SlotFit, "CHECK_EVERY", 1)
    monkeypatch.setattr(C._SlotFit, "ADOPT_AFTER", 0)
    C._slot_fits.clear()
    case, want, dev = _bwd(name)
    alt = R.reordered(case, "alt")
    adev = _dev(alt)
    _run_bwd(alt, adev)
    assert len(C._slot_fits) == 1
    fit = next(iter(C._slot_fits.values()))
    fit.pending = None
    fit.scale = [0.02] * case["L"]
    _check_bwd(alt, want, adev, f"{name}: slots at 2 %", seeded=(False,))
    fit.scales(case["n"])                                    # collects the statistics of that launch
    st = fit.last
    print("forced:", st)
    assert st is not None and any(f >= c for f, c, b in zip(st["fill"], st["cap"], st["base"]) if b > 0), st
    assert all(c < b for c, b in zip(st["cap"], st["base"]) if b > 0), st
    # seeded as well, with the slots still small
    fit.pending = None
    fit.scale = [0.02] * case["L"]
    _check_bwd(alt, want, adev, f"{name}: slots at 2 %", seeded=(True,))
    # the run order with unscaled slots: nothing overflows (the no-merge order sends 8192 records per piece and level, more than
    # the 2048 a slot of a one-bucket dense level ever holds)
    fit.pending = None
    fit.scale = [1.0] * case["L"]
    _check_bwd(case, want, dev, f"{name}: unscaled slots", seeded=(False,))
    fit.scales(case["n"])
    st = fit.last
    print("unscaled:", st)
    assert st is not None and all(f < c for f, c, b in zip(st["fill"], st["cap"], st["base"]) if b > 0), st
    assert any(b > 0 for b in st["base"])
    C._slot_fits.clear()


@pytest.mark.parametrize("name", R.LOSS_NAMES)
def test_backward_under_a_loss_scale(name):
    """the same integer gradients times 2^16, 2^24 and 2^-30 (fp16: from a unit of 2^-10, no 2^-30): the scaled reference bit for
    bit on every level, the atomic-flushed coarse ones included"""
    for case, e in R.loss_scale_cases(name):
        _describe(case)
        want = R.reference_backward(case)["grad"]
        assert float(want.abs().max()) > 0
        _check_bwd(case, want, _dev(case), seeded=(False,))


@pytest.mark.parametrize("name", R.BIG_NAMES)
def test_backward_of_a_large_launch(name):
    """n = 2^20 + 2048 + 17 in bf16 with F = 2 (the 1024-thread wide emitter, capped grid with several pieces per workgroup) and
    n = 2^21 + 65 in fp32 (extra_bits = 1: the binary point moves up).  Two levels each, so that the float64 reference stays cheap:
    measured on an MI355X machine, reference included, the bf16 test took 1.1 s and the fp32 test 2.3 s."""
    case, want, dev = _bwd(name)
    _check_bwd(case, want, dev, seeded=(False,))
    _cache.pop(("bwd", case["name"]))
    R._cases.pop(name)


# ---------------------------------------------------------------------------------------------------- grad_coords
@pytest.mark.parametrize("F", [2, 4])
@pytest.mark.parametrize("dtype", R.FWD_DTYPES)
def test_grad_coords_equals_float64_reference(dtype, F):
    """the reference's arithmetic, quirks included, at n = 1, 255, 256 and 257; 2-D returns the zero [n, 3] tensor"""
    C = _C()
    for n in R.GC_N:
        for dim in (3, 2):
            case = R.grad_coords_case(dtype, F, n, dim)
            _describe(case)
            dev = _dev(case)
            got = C.hashgrid_grad_coords(dev["coords"], dev["grad_out"], dev["table"], dev["first_idx"], case["res"], case["bitwidth"])
            torch.cuda.synchronize()
            want = R.reference_grad_coords(case)
            _same(got, want, case["name"])
            assert (dim == 2) == (int(got.count_nonzero()) == 0)


# ---------------------------------------------------------------------------------------------------- corner query
@pytest.mark.parametrize("probe_bitwidth", [0, 1])
@pytest.mark.parametrize("dtype", R.FWD_DTYPES)
def test_query_backward_equals_float64_reference(dtype, probe_bitwidth):
    """fp32: probe p into row idx + p; fp16 / bf16: packed atomics, every probe into row idx"""
    case = R.make_query_case(dtype, probe_bitwidth)
    print(f"{case['name']}: n = {case['n']}, levels {case['res']}, bitwidth {case['bitwidth']}")
    want = R.reference_query_backward(case)
    td = R.DTYPES[dtype]
    g = case["grad_out"].float().to(td).reshape(case["n"], 8, -1).to(DEV)
    got = _C().hashgrid_query_backward(case["coords"].to(DEV), g, case["res"], [2 ** case["bitwidth"]] * case["L"], case["bitwidth"],
                                       case["F"], probe_bitwidth)
    torch.cuda.synchronize()
    for l, (a, b) in enumerate(zip(got, want)):
        _same(a, b, f"{case['name']} level {l}")


# ---------------------------------------------------------------------------------------------------- environment switches
SWITCHES = [{"WISP_HG_BWD_MERGE": "0"}, {"WISP_HG_BWD_BIN": "0"}, {"WISP_HG_BWD_QUEUE": "0", "WISP_HG_STRIP_BUCKETS": "0"},
            {"WISP_HG_EMIT_SMALL_BELOW": "0", "WISP_HG_EMIT_WIDE": "0"}]


@pytest.mark.parametrize("switches", SWITCHES, ids=lambda s: ",".join(f"{k}={v}" for k, v in s.items()))
def test_backward_under_environment_switches(switches):
    """hashgrid.hip reads its switches once per process, so each setting runs the backward case list in a fresh child process
    (tests/hashgrid_exact_worker.py): no merge; no bins; the generic emitter and consecutive-row buckets for everything; the
    512-thread queue emitter, which nothing reaches by default"""
    env = dict(os.environ)
    env.update(switches)
    worker = os.path.join(os.path.dirname(os.path.abspath(__file__)), "hashgrid_exact_worker.py")
    done = subprocess.run([sys.executable, worker], env=env, timeout=420, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    print(done.stdout)
    assert done.returncode == 0, f"worker exit status {done.returncode} under {switches}:\n{done.stdout}"
    lines = [json.loads(l) for l in done.stdout.splitlines() if l.startswith("{")]
    assert [l["name"] for l in lines] == list(R.BWD_NAMES) and all(l["ok"] for l in lines)
