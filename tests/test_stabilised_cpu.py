"""Stabilised saddle-point systems [[A, B^T], [B, C]] without a GPU: the generator of C, the entry points' protocol
path on the numpy engine against the goldens of the reference's own files (tests/golden/make_stabilised_golden.py),
and what the fused loops answer when they are offered a C."""

import numpy as np
import pytest
import scipy.sparse as sp

import stabilised_cases as sc
from staggered_grid import mac_stokes


@pytest.mark.parametrize("name", sc.NAMES)
def test_protocol_path_reproduces_the_goldens(numpy_engine, name):
    """`bramble_pasciak_cg(a, b, c, ...)` and `MinRes(mat=[[A, B^T], [B, C]])` statement by statement: history to 1e-8
    over the fixture's stable window, iterations inside conftest.iteration_tolerance, the residual with C."""
    d = sc.load(name)
    case = sc.StabCase(d)
    assert (case.system.n_u, case.system.n_p) == (int(d["n_u"]), int(d["n_p"]))
    sc.run_entry_point(d, case, sc.device_operands(case))


def test_a_well_shaped_c_reaches_the_engine_check(numpy_engine):
    """An n_p x n_p SparseMatrix in the C slot is no longer a reason to decline: on the numpy engine both loops now
    decline for the engine's sake.  Anything else in the slot keeps the reason it had."""
    import hipla
    from hipla import fused
    case = sc.StabCase(sc.params(2, 3, 0.5, "jacobi"))
    s = case.system
    A, B, Cm, preA, preS = sc.device_operands(case)

    def block():
        return hipla.BlockVector([hipla.Vector(s.n_u), hipla.Vector(s.n_p)])

    def minres(c):
        K = hipla.BlockMatrix([[A, B.T], [B, c]])
        P = hipla.BlockMatrix([[preA, None], [None, preS]])
        rings = [block() for _ in range(3)], [block() for _ in range(3)], [block() for _ in range(2)]
        assert fused.MinresLoop.try_create(K, P, block(), *rings, block()) is None
        return fused.MinresLoop.last_declined

    def bpcg1(c):
        vecs = {name: block() for name in ("x", "r", "d", "a", "t1", "t2")}
        assert fused.Bpcg1Loop.try_create(A, B, c, preA, preS, 1.0, vecs) is None
        return fused.Bpcg1Loop.last_declined

    assert minres(Cm) == "not the HIP engine" and bpcg1(Cm) == "not the HIP engine"
    assert minres(None) == "not the HIP engine" and bpcg1(None) == "not the HIP engine"

    class Opaque(hipla.BaseMatrix):
        def Height(self):
            return s.n_p

        def Width(self):
            return s.n_p

    wide = hipla.SparseMatrix.from_scipy(sp.csr_matrix((s.n_p, s.n_p + 1)))
    for other in (A, wide, Opaque(), hipla.DiagonalMatrix(np.ones(s.n_p)), 2.0 * Cm):
        assert minres(other) == "K or C has another non-zero block"
        assert bpcg1(other) == "C is given"


@pytest.mark.parametrize("dim,n", [(2, 3), (3, 2)])
def test_pressure_stabilisation_against_dense_loops(dim, n):
    """C = -eps h^(2 - dim) B B^T: entry by entry from loops over the cells and their interior faces (a face of area
    h^(dim-1) between the cells i and j contributes -w to C_ii and C_jj and +w to C_ij, w = eps h^dim), symmetric,
    sorted, and zero on the constants up to the rounding of the row sums."""
    s = mac_stokes(dim, n, 0.01)
    eps = 0.75
    C = s.pressure_stabilisation(eps)
    assert sp.isspmatrix_csr(C) and C.shape == (s.n_p, s.n_p) and C.has_sorted_indices
    w = eps * s.h ** dim
    want = np.zeros((s.n_p, s.n_p))
    cells = np.arange(s.n_p).reshape((n,) * dim)
    for idx in np.ndindex(*cells.shape):
        for ax in range(dim):
            if idx[ax] + 1 < n:
                nb = list(idx)
                nb[ax] += 1
                i, j = cells[idx], cells[tuple(nb)]
                want[i, i] -= w
                want[j, j] -= w
                want[i, j] += w
                want[j, i] += w
    got = C.toarray()
    # each entry of B B^T is a sum of at most 2 dim equal products, then one product with the factor: a few roundings
    assert np.abs(got - want).max() <= 8 * np.finfo(float).eps * np.abs(want).max()
    assert np.array_equal(got != 0.0, want != 0.0)
    assert np.array_equal(got, got.T)
    assert np.abs(C @ np.ones(s.n_p)).max() <= 8 * np.finfo(float).eps * np.abs(want).max()
    assert np.all(np.linalg.eigvalsh(got) <= 1e-14 * np.abs(want).max())


def test_pressure_stabilisation_wants_a_plain_system():
    s = mac_stokes(2, 4, 0.01).inflate(2)
    with pytest.raises(ValueError, match="plain systems only"):
        s.pressure_stabilisation(1.0)
