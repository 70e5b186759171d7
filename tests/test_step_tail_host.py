"""CPU: the float32 restatements of the step's two closing sums (tests/step_tail_ref.py; kernels: csrc/step_tail_dev.h) against float64.
A float32 sum of n terms in ANY order differs from the exact sum by at most (n - 1) u sum|x| (1 + O(n u)), u = 2^-24 (Higham, Accuracy
and Stability of Numerical Algorithms, eq. 4.4); the bound asserted here is n 2^-24 sum|x| - the float64 reference's own error
(n 2^-53 sum|x|) and the second-order term are far below the slack between n - 1 and n at these sizes."""
import numpy as np
import pytest

import step_tail_ref as R

U = 2.0 ** -24


@pytest.mark.parametrize("rows", [1, 15, 16, 17, 256])
@pytest.mark.parametrize("in_dim", [32, 30])
def test_dw_restatement_against_float64(rows, in_dim):
    rng = np.random.default_rng(rows * 100 + in_dim)
    partials = np.zeros((rows, R.NPARAM_PAD), dtype=np.float32)
    partials[:, :R.NPARAM] = rng.normal(size=(rows, R.NPARAM)).astype(np.float32) * rng.choice([1e-3, 1.0, 50.0], size=(rows, 1)).astype(np.float32)
    packed = R.NPARAM - R.H * (R.IN - in_dim)
    before = rng.normal(size=packed).astype(np.float32)
    got = R.dw_reduce(partials, rows, in_dim, before)
    dst = R.packed_index(in_dim)
    keep = dst >= 0
    assert got.dtype == np.float32 and int(keep.sum()) == packed and sorted(dst[keep].tolist()) == list(range(packed))
    exact = before.astype(np.float64)
    exact[dst[keep]] += partials[:, :R.NPARAM].astype(np.float64).sum(0)[keep]
    mag = np.abs(before.astype(np.float64))
    mag[dst[keep]] += np.abs(partials[:, :R.NPARAM].astype(np.float64)).sum(0)[keep]
    n = rows + 1                                            # the addends of one element: its rows and what grad_params held
    assert np.all(np.abs(got.astype(np.float64) - exact) <= n * U * mag)
    # a padding column of W1 (in_dim 30: columns 30, 31) reaches nothing
    if in_dim < R.IN:
        assert int((~keep).sum()) == R.H * (R.IN - in_dim)


def test_dw_restatement_order_is_the_kernels():
    """values chosen so that the order shows: 2^24 and ones - rows 0 and 16 share a group, row 1 does not"""
    partials = np.zeros((17, R.NPARAM_PAD), dtype=np.float32)
    partials[0, 5] = 2.0 ** 24
    partials[16, 5] = 1.0            # group 0: 2^24 + 1 -> 2^24 (rounds to even)
    partials[1, 5] = 1.0             # group 1: 1
    got = R.dw_reduce(partials, 17, 32, np.zeros(R.NPARAM, dtype=np.float32))
    assert got[5] == np.float32(2.0 ** 24)                  # (2^24 + 1 -> 2^24) + 1 -> 2^24; any exact or pairwise order gives 2^24 + 2
    partials[16, 5], partials[2, 5] = 0.0, 1.0              # now three ones in groups 1 and 2: still lost one at a time
    assert R.dw_reduce(partials, 17, 32, np.zeros(R.NPARAM, dtype=np.float32))[5] == np.float32(2.0 ** 24)
    partials[0, 5], partials[15, 5] = 0.0, 2.0 ** 24        # the large term LAST: 1 + 1 first, then + 2^24 = 2^24 + 2 exactly
    assert R.dw_reduce(partials, 17, 32, np.zeros(R.NPARAM, dtype=np.float32))[5] == np.float32(2.0 ** 24 + 2.0)


@pytest.mark.parametrize("n", [0, 1, 4, 63, 64, 1024, 1025, 4096, 4097, 8192, 8193, 20000])
def test_loss_restatement_against_float64(n):
    rng = np.random.default_rng(n + 7)
    x = (rng.uniform(0.0, 1.5, size=n) * rng.choice([1e-4, 1.0, 30.0], size=n)).astype(np.float32)
    inv_n = np.float32(1.0 / max(3 * n, 1))
    got = R.loss_sum(x, inv_n)
    assert isinstance(got, np.float32)
    exact = float(x.astype(np.float64).sum()) * float(inv_n)
    bound = (n + 1) * U * float(np.abs(x.astype(np.float64)).sum()) * float(inv_n)       # n terms and the final product
    assert abs(float(got) - exact) <= bound, (float(got), exact, bound)


def test_loss_restatement_order_is_the_kernels():
    """thread 0 of wave 0 adds partial[0], partial[1024], ...; lane 0 takes lane 32 first"""
    x = np.zeros(2048, dtype=np.float32)
    x[0], x[1024] = 2.0 ** 24, 1.0                          # same thread: 2^24 + 1 -> 2^24
    x[32] = 1.0                                             # lane 32 of the same wave: folded in first -> + 1 lost again
    assert R.loss_sum(x, 1.0) == np.float32(2.0 ** 24)
    x[1024], x[33] = 0.0, 1.0                               # lane 32 folds into lane 0 and lane 33 into lane 1 at offset 32:
    assert R.loss_sum(x, 1.0) == np.float32(2.0 ** 24)      # 2^24 + 1 -> 2^24; lane 1 joins at offset 1: + 1 -> 2^24 again
    x[0], x[64] = 0.0, 2.0 ** 24                            # the large term in wave 1: wave 0 sums 1 + 1 = 2 first, 2 + 2^24 exact
    assert R.loss_sum(x, 0.5) == np.float32((2.0 ** 24 + 2.0) * 0.5)
