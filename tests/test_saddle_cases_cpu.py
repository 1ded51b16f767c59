"""The oracle alone on the systems of tests/saddle_cases.py: the conditions tests/test_saddle_loop_edges_gpu.py rests on.
Point Jacobi for A, the inverse of `mass` for the Schur complement, at every size of `SIZES`:

* BPCG v2, the textbook BPCG and MINRES converge to 1e-10 in fewer than 500 iterations (measured: 2 to 335) and end within
  1e-9 relative of the dense solve of [[A, B^T], [B, 0]] (measured: at most 7.1e-10);
* the first three iterates of each method move by at most 1e-12 relative when the problem is symmetrically permuted --
  the same problem with different rounding (measured: at most 5.8e-16).  The GPU tests hold the fused loops to 1e-11."""

import numpy as np
import pytest

import saddle_cases as sc
from oracle import krylov_ref as kr


def operands(n_u, n_p):
    A, B, f, g, mass = sc.case(n_u, n_p)
    pa, ps = kr.jacobi(A), kr.diag_inverse(mass)
    return (A, B, f, g), pa, ps, sc.scale(A, pa)


def test_the_systems_are_what_the_gpu_tests_assume():
    empty_rows = 0
    for n_u, n_p in sc.SIZES:
        A, B, f, g, mass = sc.case(n_u, n_p)
        assert A.shape == (n_u, n_u) and B.shape == (n_p, n_u) and A.has_sorted_indices
        assert abs(A - A.T).max() == 0.0 and np.linalg.eigvalsh(A.toarray())[0] > 0.0
        lam = np.linalg.eigvals(A.toarray() / A.diagonal()[:, None]).real
        assert 0.7 < lam.min() and lam.max() < 1.3
        assert np.linalg.matrix_rank(B.toarray()) == n_p
        assert 0.5 <= mass.min() and mass.max() < 1.5
        empty_rows += int(np.diff(B.T.tocsr().indptr).min() == 0)
        if n_u > 3:
            lens = np.diff(A.indptr)
            assert lens.min() >= 1 and lens.max() > 2            # ragged rows
    assert empty_rows >= len(sc.SIZES) // 2                      # B^T has empty rows at most sizes
    assert sc.runs(5, [2]) == [[0, 1], [2, 3], [4]] and sc.runs(7, [1, 2, 3]) == [[0], [1, 2], [3, 4, 5], [6]]
    assert [len(sc.runs(n, [2])) for n in (65, 511, 513, 1025)] == [33, 256, 257, 513]


@pytest.mark.parametrize("size", sc.SIZES, ids=lambda s: "%dx%d" % s)
def test_the_reference_converges_to_the_dense_solve(size):
    ops, pa, ps, k = operands(*size)
    exact = sc.dense_solution(*ops)
    for method in sc.METHODS:
        count, x, hist = sc.reference(method, ops, pa, ps, k, 1e-10, 500)
        err = sc.distance(x, exact)
        print("%s at %s: %d iterations, %.3g from the dense solve" % (method, size, count, err))
        assert 0 < count < 500
        assert err <= 1e-9


@pytest.mark.parametrize("size", sc.SIZES, ids=lambda s: "%dx%d" % s)
def test_a_permutation_moves_the_first_iterates_by_rounding_only(size):
    ops, pa, ps, k = operands(*size)
    A, B, f, g, mass = sc.case(*size)
    (Ap, Bp, fp, gp, massp), (pi, sigma) = sc.permuted(A, B, f, g, mass, seed=7)
    twin, pap, psp = (Ap, Bp, fp, gp), kr.jacobi(Ap), kr.diag_inverse(massp)
    order = np.concatenate([pi, A.shape[0] + sigma])
    for method in sc.METHODS:
        needed = sc.reference(method, ops, pa, ps, k, 1e-10, 500)[0]
        for steps in range(1, min(3, needed - 1) + 1):
            x = sc.reference(method, ops, pa, ps, k, 0.0, steps)[1]
            xp = sc.reference(method, twin, pap, psp, k, 0.0, steps)[1]
            moved = sc.distance(xp, x[order])
            print("%s at %s, iterate %d: moved by %.3g" % (method, size, steps, moved))
            assert moved <= 1e-12
