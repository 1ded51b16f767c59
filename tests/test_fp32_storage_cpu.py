"""storage="fp32" of the preconditioners (BlockGaussSeidel, SmoothedAggregationAMG, AuxiliarySpaceAMG, MypreA) on the
numpy checker engine: the option gives the fp64 operator of the matrices rounded once to fp32 (kept in float64 here),
"fp64" and no option build identical operators, invalid values raise, and the fused loops' decoder classifies fp32
handles exactly as their fp64 twins."""
import numpy as np
import pytest

from oracle import krylov_ref as kr


def _round32(m):
    import scipy.sparse as sp
    out = sp.csr_matrix(m, copy=True)
    out.data = out.data.astype(np.float32).astype(np.float64)
    return out


def _apply(op, x):
    import hipla
    xv = hipla.Vector.from_numpy(x)
    yv = hipla.Vector(op.Height())
    op.Mult(xv, yv)
    return yv.numpy()


def _stokes(n=6):
    from staggered_grid import mac_stokes
    return mac_stokes(3, n, 0.01)


def _perturbed(A):
    """A with values that are not representable in fp32 (so rounding shows)."""
    import scipy.sparse as sp
    A = sp.csr_matrix(A, copy=True)
    A = A + A.T.multiply(1e-9 * np.pi)          # symmetric, full-precision entries
    A.sort_indices()
    return A.tocsr()


def test_block_gauss_seidel_fp32_is_the_operator_of_round32(numpy_engine):
    import hipla
    s = _stokes()
    Ah = _perturbed(s.A)
    A = hipla.SparseMatrix.from_scipy(Ah)
    blocks = s.line_blocks(3)
    G32 = hipla.BlockGaussSeidel(A, blocks, storage="fp32")
    G64 = hipla.BlockGaussSeidel(A, blocks)
    assert G32.storage == "fp32" and G64.storage == "fp64"
    assert G32.mat is A                                         # the loop's matrix is not touched
    np.testing.assert_array_equal(A.to_scipy().data, Ah.data)
    x = np.random.default_rng(0).standard_normal(s.n_u)
    ref = kr.symmetric_block_gauss_seidel(_round32(Ah), G32.idx_host)(x)
    y = _apply(G32, x)
    assert np.linalg.norm(y - ref) <= 1e-12 * np.linalg.norm(ref)
    y64 = _apply(G64, x)
    d = np.linalg.norm(y - y64) / np.linalg.norm(y64)
    assert 1e-12 < d < 1e-5, d                                  # the rounded operator really is applied


def test_amg_fp32_is_the_cycle_of_the_rounded_hierarchy(numpy_engine):
    import hipla
    s = _stokes(8)
    A = hipla.SparseMatrix.from_scipy(_perturbed(s.A))
    V32 = hipla.SmoothedAggregationAMG(A, coarse_size=50, storage="fp32")
    V64 = hipla.SmoothedAggregationAMG(A, coarse_size=50)
    assert len(V32.levels) >= 2
    for l32, l64 in zip(V32.applied_levels, V32.levels):
        for key in ("A", "P", "R"):
            if key in l64:
                np.testing.assert_array_equal(l32[key].to_scipy().toarray(), _round32(l64[key].to_scipy()).toarray())
        assert l32["dinv"] is l64["dinv"]                        # smoother diagonals and the coarse inverse: fp64
        if "inv" in l64:
            assert l32["inv"] is l64["inv"]
    x = np.random.default_rng(1).standard_normal(s.n_u)
    y32, y64 = _apply(V32, x), _apply(V64, x)
    d = np.linalg.norm(y32 - y64) / np.linalg.norm(y64)
    assert 1e-12 < d < 1e-5, d
    r = np.random.default_rng(2).standard_normal(s.n_u)
    assert abs(r @ y32 - x @ _apply(V32, r)) <= 1e-12 * np.linalg.norm(y32) * np.linalg.norm(r)   # symmetric


def test_fp64_storage_and_no_option_are_identical(numpy_engine):
    import hipla
    s = _stokes()
    A = hipla.SparseMatrix.from_scipy(_perturbed(s.A))
    blocks = s.line_blocks(3)
    x = np.random.default_rng(3).standard_normal(s.n_u)
    V = hipla.SmoothedAggregationAMG(A, coarse_size=50)
    np.testing.assert_array_equal(_apply(hipla.BlockGaussSeidel(A, blocks, storage="fp64"), x),
                                  _apply(hipla.BlockGaussSeidel(A, blocks), x))
    np.testing.assert_array_equal(_apply(hipla.BlockGaussSeidel(A, blocks, middle=V, storage="fp64"), x),
                                  _apply(hipla.BlockGaussSeidel(A, blocks, middle=V), x))
    np.testing.assert_array_equal(_apply(hipla.SmoothedAggregationAMG(A, coarse_size=50, storage="fp64"), x),
                                  _apply(V, x))
    assert hipla.SmoothedAggregationAMG(A, coarse_size=50).applied_levels is not None


@pytest.mark.parametrize("bad", ["fp16", "float32", "FP32", None, 32])
def test_invalid_storage_raises(numpy_engine, bad):
    import hipla
    s = _stokes(4)
    A = hipla.SparseMatrix.from_scipy(s.A)
    with pytest.raises(ValueError):
        hipla.BlockGaussSeidel(A, s.line_blocks(3), storage=bad)
    with pytest.raises(ValueError):
        hipla.SmoothedAggregationAMG(A, storage=bad)
    with pytest.raises(ValueError):
        hipla.Preconditioner(A, "h1amg", storage=bad)
    with pytest.raises(ValueError):
        hipla.Preconditioner(A, "local", storage="fp32")        # stores no matrix of its own


def test_preconditioner_honours_storage(numpy_engine):
    import hipla
    s = _stokes(6)
    A = hipla.SparseMatrix.from_scipy(_perturbed(s.A))
    for kind in ("h1amg", "multigrid"):
        assert hipla.Preconditioner(A, kind, storage="fp32").storage == "fp32"
        assert hipla.Preconditioner(A, kind).storage == "fp64"


def _mypre(storage, gs, condense=False):
    from templates.NavierStokesSIMPLE_iterative import (AssembledForm, MypreA, NavierStokes, SyntheticMesh,
                                                         auxiliary_space_preconditioner)
    ns = NavierStokes(SyntheticMesh(1.0 / 5, dim=3), nu=0.01, inflow="inlet", outflow="outlet", wall="wall|cyl",
                      uin=None, timestep=0.001, order=1)
    _, _, aux = auxiliary_space_preconditioner(ns.system, storage=storage)
    return ns, aux, MypreA(ns.V, AssembledForm(ns.a.mat), ns.system.facet_blocks(), GS=gs, aux=aux, storage=storage)


@pytest.mark.parametrize("gs", [True, False])
def test_mypre_a_fp32_symmetric_and_rounded(numpy_engine, gs):
    ns, aux, P32 = _mypre("fp32", gs)
    _, _, P64 = _mypre("fp64", gs)
    n = P32.Height()
    rng = np.random.default_rng(4)
    x, y = rng.standard_normal(n), rng.standard_normal(n)
    px, py = _apply(P32, x), _apply(P32, y)
    assert abs(px @ y - x @ py) <= 1e-13 * np.linalg.norm(px) * np.linalg.norm(y)
    d = np.linalg.norm(px - _apply(P64, x)) / np.linalg.norm(px)
    # GS=True: A's values are not fp32 numbers, the rounded sweep shows; GS=False: the additive block Jacobi stores no
    # matrix and the auxiliary-space operators of this grid (T, the Laplacians) are fp32 numbers already
    assert (1e-10 < d < 1e-5) if gs else d < 1e-5, d
    assert aux.storage == "fp32"


@pytest.mark.parametrize("gs", [True, False])
def test_decoder_classifies_fp32_handles_as_their_fp64_twins(numpy_engine, gs):
    from hipla import fused
    _, _, P32 = _mypre("fp32", gs)
    _, _, P64 = _mypre("fp64", gs)
    p32, p64 = fused.native_velocity_pre(P32), fused.native_velocity_pre(P64)
    assert p32 is not None and p64 is not None
    assert (p32.scale, p32.multiplicative, p32.diag is None, type(p32.bjac), type(p32.amg)) == \
           (p64.scale, p64.multiplicative, p64.diag is None, type(p64.bjac), type(p64.amg))
    for name, accepts in fused.ACCEPTS.items():
        assert accepts(p32) == accepts(p64), name
    assert fused.fp32_storage(p32) and not fused.fp32_storage(p64)
    if gs:
        assert fused.own_residual_matrix(p32.bjac) is not None and fused.own_residual_matrix(p64.bjac) is None


def test_solve_initial_pre_storage_on_the_checker(numpy_engine):
    """SolveInitial(pre_storage="fp32") converges like the fp64 run (both forms): the option is plumbed through."""
    import contextlib
    import io
    from templates.NavierStokesSIMPLE_iterative import NavierStokes, SyntheticMesh
    its = {}
    for condense in (False, True):
        for storage in ("fp64", "fp32"):
            ns = NavierStokes(SyntheticMesh(1.0 / 5, dim=3), nu=0.01, inflow="inlet", outflow="outlet",
                              wall="wall|cyl", uin=None, timestep=0.001, order=1)
            with contextlib.redirect_stdout(io.StringIO()):
                ns.SolveInitial(iterative=True, GS=True, tol=1e-8, maxsteps=3000, condense=condense,
                                pre_storage=storage)
            assert ns.preA.storage == storage
            its[condense, storage] = ns.stokes_bpcg_iterations
        a, b = its[condense, "fp64"], its[condense, "fp32"]
        assert abs(a - b) <= max(3, int(0.03 * a)), its
