"""The yardstick of tests/test_gpu_lu.py checked on the host (no GPU): for every (family, C) the GPU file uses up to C = 200, and
for `sign` and `graded` at C = 512,
  * cond_2(W) <= 2e4 (the bounds of lu_oracle assume the fp64 factorisation error is negligible beside one fp32 ulp), and
  * numpy's fp64 slogdet / inv agree with an independent long-double Gauss-Jordan (partial pivoting, np.longdouble) to 1e-2 of the
    bounds the kernels are held to (lu_oracle.logdet_bound, inverse_bound).
Measured over all six families at C in {12 ... 512}: worst log-det error 6.6e-4 of its bound, worst inverse error 6.7e-4 of its bound
(both `graded`, C = 448 / 512); cond reaches 2.5e3 (`orth`, C = 448) and 1.1e4 (`sign`, C = 512)."""
import numpy as np
import pytest

import lu_oracle as LU

CASES = LU.host_checked_cases()


@pytest.mark.parametrize("family,C", CASES, ids=[f"{f}-{C}" for f, C in CASES])
def test_fp64_reference_against_long_double_gauss_jordan(family, C):
    W = LU.matrix(family, C)
    assert W.dtype == np.float32 and W.shape == (C, C) and np.isfinite(W).all()
    cond = np.linalg.cond(W.astype(np.float64))
    assert cond <= LU.COND_MAX, cond
    ld, inv = LU.reference(family, C)
    ld_x, inv_x = LU.longdouble_gauss_jordan(W)
    e_ld = abs(float(np.longdouble(ld) - ld_x)) / LU.logdet_bound(ld)
    e_inv = float((np.abs(inv.astype(np.longdouble) - inv_x).astype(np.float64) / LU.inverse_bound(inv)).max())
    print(f"{family} C={C}: cond {cond:.3g}  logdet {ld:.6g} err {e_ld:.2e} of bound  inverse err {e_inv:.2e} of bound")
    assert e_ld <= 1e-2 and e_inv <= 1e-2, (e_ld, e_inv)


@pytest.mark.parametrize("C", [1, 3, 12, 64, 66, 130, 200, 512])
def test_cyclic_is_exact_and_swaps_with_the_last_row_at_every_step(C):
    """The closed form IS what numpy's fp64 routines return (value for value: every operation on powers of two is exact), and the
    family does what it is for: at every step the only candidate at or below the diagonal is the last row."""
    W = LU.matrix("cyclic", C)
    ld, inv = LU.reference("cyclic", C)
    ld_x, inv_x = LU.cyclic_exact(C, LU.SEED)
    assert np.array_equal(inv, inv_x) and abs(ld - ld_x) <= 1e-12 * max(1.0, abs(ld_x))
    assert np.array_equal(inv_x.astype(np.float32).astype(np.float64), inv_x)      # W^-1 is exact in float32 too
    A = W.astype(np.float64).copy()
    for k in range(C - 1):
        assert np.flatnonzero(A[k:, k]).tolist() == [C - 1 - k], k
        A[[k, C - 1]] = A[[C - 1, k]]


def test_families_do_what_they_are_for():
    for C in (66, 130, 200):
        W = LU.matrix("anti", C).astype(np.float64)
        assert all(int(np.argmax(np.abs(W[:, k]))) == C - 1 - k for k in range(C))          # pivots from the mirrored rows
        S = LU.matrix("sign", C)
        assert set(np.unique(S).tolist()) == {-1.0, 1.0}
        assert abs(LU.reference("graded", C)[0]) < 1e-3 * C                                   # log|det| ~ 0: the floor decides
    with np.errstate(over="ignore", under="ignore"):
        assert not np.isfinite(np.float32(np.prod(np.abs(np.linalg.eigvals(LU.matrix("sign", 64).astype(np.float64))).astype(np.float32))))
        assert np.linalg.det(LU.matrix("tiny", 128).astype(np.float64)) == 0.0              # fp64 `det` underflows from C = 128
        assert np.float32(np.linalg.det(LU.matrix("tiny", 24).astype(np.float64))) == 0.0   # fp32 from C = 24
    assert abs(LU.reference("tiny", 128)[0] + 128 * np.log(1e3)) < 1e-3
    assert 1200 < LU.reference("sign", 512)[0] < 1500
