"""storage="fp32" on the MI355X: the Gauss-Seidel sweep, the V-cycle and the auxiliary-space term streaming 4-byte
values (nss_csr_narrow_f32), the multiplicative and additive MypreA, the default SolveInitial (both forms) and the
fused CG / MINRES loops with fp32 handles -- against the operators of the rounded matrices and against fp64 runs."""
import contextlib
import io
import re

import numpy as np
import pytest

from oracle import krylov_ref as kr
from staggered_grid import mac_stokes

pytestmark = pytest.mark.gpu


def _round32(m):
    import scipy.sparse as sp
    out = sp.csr_matrix(m, copy=True)
    out.data = out.data.astype(np.float32).astype(np.float64)
    return out


def _perturbed(A):
    """A (symmetric) with values that are not fp32 numbers."""
    import scipy.sparse as sp
    A = sp.csr_matrix(A, copy=True)
    A = (A + A.T.multiply(1e-9 * np.pi)).tocsr()
    A.sort_indices()
    return A


def _apply(op, x):
    import hipla
    y = hipla.Vector(op.Height())
    op.Mult(hipla.Vector.from_numpy(x), y)
    return y.numpy()


def _rel(a, b):
    return np.linalg.norm(a - b) / np.linalg.norm(b)


@pytest.mark.parametrize("uncovered", [False, True])
def test_block_gauss_seidel_fp32_against_the_rounded_sweep(hip_engine, uncovered):
    import hipla
    from hipla.matrix import value_bytes
    s = mac_stokes(3, 8, 0.01)
    Ah = _perturbed(s.A)
    A = hipla.SparseMatrix.from_scipy(Ah)
    blocks = s.line_blocks(3)
    if uncovered:                                               # every fifth block dropped: dofs in no block
        blocks = blocks[:, np.arange(blocks.shape[1]) % 5 != 0]
    G = hipla.BlockGaussSeidel(A, blocks, storage="fp32")
    assert G.layout == "colour-major"
    assert (G.n_uncovered > 0) == uncovered
    x = np.random.default_rng(0).standard_normal(s.n_u)
    y = _apply(G, x)
    ref = kr.symmetric_block_gauss_seidel(_round32(Ah), G.idx_host)(x)
    assert _rel(y, ref) <= 1e-12
    assert _rel(y, _apply(hipla.BlockGaussSeidel(A, blocks), x)) > 1e-12     # the rounded matrix is what is applied
    assert value_bytes(G.perm_handle, G.engine) == 4 * G.perm_handle.nnz
    np.testing.assert_array_equal(A.to_scipy().data, Ah.data)                  # the caller's matrix is untouched
    # the row-permuted layout takes the fp32 sweep matrix too
    R = hipla.BlockGaussSeidel(A, blocks, layout="rows", storage="fp32")
    assert _rel(_apply(R, x), kr.symmetric_block_gauss_seidel(_round32(Ah), R.idx_host)(x)) <= 1e-12


def test_narrowed_matrix_spmv_readback_and_refusals(hip_engine):
    import hipla
    from hipla.matrix import fp32_copy, value_bytes
    from hipla.hip_engine import NssError
    s = mac_stokes(3, 8, 0.01)
    Ah = _perturbed(s.A)
    A = hipla.SparseMatrix.from_scipy(Ah)
    A32 = fp32_copy(A)
    assert value_bytes(A32) == 4 * A.nnz and value_bytes(A) == 8 * A.nnz
    np.testing.assert_array_equal(A32.to_scipy().toarray(), _round32(Ah).toarray())   # widened read-back
    x = np.random.default_rng(1).standard_normal(s.n_u)
    assert _rel(_apply(A32, x), _round32(Ah) @ x) <= 1e-14
    with pytest.raises(NssError):                               # set-up paths take fp64 values only
        hip_engine.csr_transpose(A32.handle)
    with pytest.raises(NssError):
        hip_engine.bjac_create(A32.handle, s.line_blocks(3))


def test_narrowed_spmv_over_the_lanes_per_row_regimes_and_a_grouped_matrix(hip_engine):
    """The fp32 stream kernel at every lanes-per-row value of the launch plan, in every column form and with one 16-bit
    index per group of columns (the preconditioners only reach a few of them): against scipy on the rounded values, to
    the tolerance of the narrowed SpMV above."""
    import lane_regimes
    inflated = mac_stokes(3, 6).inflate(6).A                     # block-structured: runs of 6 consecutive columns
    seen, forms, groups = set(), set(), set()
    for name, make, lanes, form in lane_regimes.CASES + [("inflated", lambda: inflated, 4, None)]:
        mat = make()
        h = hip_engine.csr_create(mat.shape[0], mat.shape[1], mat.indptr, mat.indices, mat.data)
        hip_engine.csr_narrow_f32(h)
        info = h.info()
        assert info["lanes_per_row"] == lanes == lane_regimes.plan_lanes(mat.nnz / mat.shape[0]), (name, info)
        assert info["value_bytes"] == 4 * mat.nnz and form in (None, info["operand_form"]), (name, info)
        x = np.random.default_rng(lanes).standard_normal(mat.shape[1])
        xb, yb = hip_engine.zeros(h.n), hip_engine.zeros(h.m)
        hip_engine.upload(x, xb)
        hip_engine.csr_spmv(h, 1.0, xb, 0.0, yb)
        hip_engine.synchronize()
        assert _rel(hip_engine.to_host(yb), _round32(mat) @ x) <= 1e-14, name
        seen.add(info["lanes_per_row"])
        forms.add(info["operand_form"])
        groups.add(info["index_group"])
    assert forms >= {"gather32", "gather16", "staged"} and groups == {1, 6}
    assert seen == {1, 2, 4, 8, 16, 32, 64}


def test_amg_and_auxiliary_fp32_against_the_rounded_build(hip_engine):
    """The fp32 V-cycle and auxiliary-space term against the numpy checker engine's rounded build (same hierarchy:
    the device set-up reproduces the host one bit for bit) -- to 1e-12."""
    import hipla
    from oracle.numpy_engine import NumpyEngine
    from templates.NavierStokesSIMPLE_iterative import NavierStokes, SyntheticMesh, auxiliary_space_preconditioner
    s = mac_stokes(3, 12, 0.01)
    Ah = _perturbed(s.A)
    x = np.random.default_rng(2).standard_normal(s.n_u)
    V = hipla.SmoothedAggregationAMG(hipla.SparseMatrix.from_scipy(Ah), storage="fp32")
    assert len(V.levels) >= 2
    assert V.value_bytes() == 4 * sum(lv[k].nnz for lv in V.levels for k in ("A", "P", "R") if k in lv)
    y = _apply(V, x)
    ns = NavierStokes(SyntheticMesh(1.0 / 8, dim=3), nu=0.01, inflow="inlet", outflow="outlet", wall="wall|cyl",
                      uin=None, timestep=0.001, order=1)
    space = ns.system.auxiliary_space()
    _, _, aux = auxiliary_space_preconditioner(ns.system, space=space, storage="fp32")
    xa = np.random.default_rng(3).standard_normal(aux.Height())
    ya = _apply(aux, xa)
    prev = hipla.set_engine(NumpyEngine())
    try:
        Vh = hipla.SmoothedAggregationAMG(hipla.SparseMatrix.from_scipy(Ah), storage="fp32")
        ref = _apply(Vh, x)
        _, _, auxh = auxiliary_space_preconditioner(ns.system, space=space, storage="fp32")
        refa = _apply(auxh, xa)
    finally:
        hipla.set_engine(prev)
    assert _rel(y, ref) <= 1e-12
    assert _rel(ya, refa) <= 1e-12


class _Form:
    def __init__(self, mat):
        self.mat = mat


@pytest.mark.parametrize("K", [2, 3])
def test_joint_cycle_fp32_with_a_shared_multilevel_component(hip_engine, K):
    """AuxiliarySpaceAMG(T, [comp] * K, storage="fp32") with ONE shared multi-level fp32 hierarchy: the joint cycle
    (cycle_multi: csr_multi_kernel<K, L, Epi, float>) runs, on values that are not fp32 numbers.  Against the numpy
    checker engine's rounded build to 1e-12, and different from the fp64 twin; then inside the additive and the
    multiplicative MypreA."""
    import scipy.sparse as sp
    import hipla
    from oracle.numpy_engine import NumpyEngine
    from templates.NavierStokesSIMPLE_iterative import MypreA
    L = _perturbed(mac_stokes(3, 12, 0.01).A)                  # SPD, nc rows, values not fp32 numbers
    s = mac_stokes(3, 8, 0.01)
    Ah = _perturbed(s.A)
    nc = L.shape[0]
    rng = np.random.default_rng(5)
    rows = np.repeat(np.arange(s.n_u), 4)
    T = sp.csr_matrix((rng.standard_normal(rows.size), (rows, rng.integers(0, K * nc, rows.size))), shape=(s.n_u, K * nc))
    T.sum_duplicates()
    T.sort_indices()
    x = rng.standard_normal(s.n_u)

    def build(storage):
        comp = hipla.SmoothedAggregationAMG(hipla.SparseMatrix.from_scipy(L), coarse_size=200, storage=storage)
        aux = hipla.AuxiliarySpaceAMG(hipla.SparseMatrix.from_scipy(T), [comp] * K, storage=storage)
        return comp, aux

    comp32, aux32 = build("fp32")
    assert len(comp32.levels) >= 3                              # a multi-level shared hierarchy: cycle_multi runs
    comp64, aux64 = build("fp64")
    y32, y64 = _apply(aux32, x), _apply(aux64, x)
    assert 1e-10 < _rel(y32, y64) < 1e-5, _rel(y32, y64)
    z = rng.standard_normal(s.n_u)
    assert abs(z @ y32 - x @ _apply(aux32, z)) <= 1e-13 * np.linalg.norm(y32) * np.linalg.norm(z)
    assert aux32.value_bytes() <= 0.55 * aux64.value_bytes()
    prev = hipla.set_engine(NumpyEngine())
    try:
        ref = _apply(build("fp32")[1], x)
    finally:
        hipla.set_engine(prev)
    assert _rel(y32, ref) <= 1e-12, _rel(y32, ref)
    A = hipla.SparseMatrix.from_scipy(Ah)
    for gs in (False, True):
        P32 = MypreA(None, _Form(A), s.line_blocks(3), GS=gs, aux=aux32, storage="fp32")
        P64 = MypreA(None, _Form(A), s.line_blocks(3), GS=gs, aux=aux64)
        px, pz = _apply(P32, x), _apply(P32, z)
        assert abs(px @ z - x @ pz) <= 1e-13 * np.linalg.norm(px) * np.linalg.norm(z), gs
        assert 1e-10 < _rel(px, _apply(P64, x)) < 1e-5, gs


def _mypre(storage, gs, maxh=1.0 / 8):
    from templates.NavierStokesSIMPLE_iterative import (AssembledForm, MypreA, NavierStokes, SyntheticMesh,
                                                         auxiliary_space_preconditioner)
    ns = NavierStokes(SyntheticMesh(maxh, dim=3), nu=0.01, inflow="inlet", outflow="outlet", wall="wall|cyl",
                      uin=None, timestep=0.001, order=1)
    _, _, aux = auxiliary_space_preconditioner(ns.system, storage=storage)
    return aux, MypreA(ns.V, AssembledForm(ns.a.mat), ns.system.facet_blocks(), GS=gs, aux=aux, storage=storage)


@pytest.mark.parametrize("gs", [True, False])
def test_mypre_a_fp32_symmetric_rounded_and_smaller(hip_engine, gs):
    aux32, P32 = _mypre("fp32", gs)
    aux64, P64 = _mypre("fp64", gs)
    rng = np.random.default_rng(4)
    x, y = rng.standard_normal(P32.Height()), rng.standard_normal(P32.Height())
    px, py = _apply(P32, x), _apply(P32, y)
    assert abs(px @ y - x @ py) <= 1e-13 * np.linalg.norm(px) * np.linalg.norm(y)
    d = _rel(px, _apply(P64, x))
    # GS=True: A's values are not fp32 numbers; GS=False: the additive block Jacobi stores no matrix and the
    # auxiliary-space operators of this grid are fp32 numbers already (the term's bytes still halve)
    assert (1e-10 < d < 1e-5) if gs else d < 1e-12, d
    if gs:
        assert P32.value_bytes() + aux32.value_bytes() <= 0.6 * (P64.value_bytes() + aux64.value_bytes())
    else:
        assert aux32.value_bytes() <= 0.6 * aux64.value_bytes()


def _solve_initial(condense, storage, maxh):
    from solvers import bramblepasciak_new as bp
    from templates.NavierStokesSIMPLE_iterative import NavierStokes, SyntheticMesh
    made = []
    orig = bp.BpcgSession

    class Recording(orig):
        def __init__(self, *a, **kw):
            super().__init__(*a, **kw)
            made.append(self)
    bp.BpcgSession = Recording
    try:
        ns = NavierStokes(SyntheticMesh(maxh, dim=3), nu=0.01, inflow="inlet", outflow="outlet", wall="wall|cyl",
                          uin=None, timestep=0.001, order=1)
        out = io.StringIO()
        with contextlib.redirect_stdout(out):
            ns.SolveInitial(iterative=True, GS=True, tol=1e-8, maxsteps=5000, condense=condense, printrates=True,
                            pre_storage=storage)
    finally:
        bp.BpcgSession = orig
    ses, = made
    hist = np.array([float(m) for m in re.findall(r"it =\s+\d+\s+err =\s+(\S+)", out.getvalue())])
    return ns, ses, hist


@pytest.mark.parametrize("condense", [False, True])
def test_solve_initial_fp32_pre_storage(hip_engine, condense):
    maxh = 1.0 / 24
    runs = {st: _solve_initial(condense, st, maxh) for st in ("fp64", "fp32")}
    for st, (ns, ses, hist) in runs.items():
        assert ses.fused_declined is None and ses.fused is not None, (st, ses.fused_declined)
        assert ses.lanczos_native, st
        assert ns.preA.storage == st
        assert len(hist) > 0 and ns.stokes_bpcg_iterations < 5000, st   # converged to the requested tolerance
    it64, it32 = runs["fp64"][0].stokes_bpcg_iterations, runs["fp32"][0].stokes_bpcg_iterations
    assert abs(it32 - it64) <= max(3, int(0.03 * it64)), (it32, it64)

    def true_residual(ns):
        import scipy.sparse as sp
        A, B = ns.a.mat.to_scipy(), ns.b.mat.to_scipy()
        K = sp.bmat([[A, B.T], [B, None]]).tocsr()
        x = np.concatenate([ns.gfu.numpy(), ns.gfup.numpy()])
        b = np.concatenate([ns.f.vec.numpy(), ns.g.vec.numpy()])
        return np.linalg.norm(b - K @ x) / np.linalg.norm(b)
    assert true_residual(runs["fp32"][0]) <= 10 * true_residual(runs["fp64"][0])


def test_fused_cg_and_minres_with_fp32_handles(hip_engine):
    import hipla
    from hipla import fused
    from minres import MinRes
    s = mac_stokes(3, 12, 0.01)
    f, g = s.rhs(0)
    Ah = _perturbed(s.A)
    A, B = hipla.SparseMatrix.from_scipy(Ah), hipla.SparseMatrix.from_scipy(s.B)
    fv = hipla.Vector.from_numpy(f)

    def cg(pre):
        solver = hipla.CGSolver(A, pre=pre, precision=1e-10, maxsteps=2000)
        y = hipla.Vector(s.n_u)
        solver.Mult(fv, y)
        assert solver._fused is not None                         # the fused loop (nss_cg_*) ran
        return solver.iterations, np.asarray(solver.errors), y.numpy()

    for make in (lambda st: hipla.SmoothedAggregationAMG(A, storage=st),
                 lambda st: hipla.BlockGaussSeidel(A, s.line_blocks(3), storage=st)):
        it64, e64, y64 = cg(make("fp64"))
        it32, e32, y32 = cg(make("fp32"))
        assert abs(it32 - it64) <= max(3, int(0.03 * it64)), (it32, it64)
        w = min(10, len(e64), len(e32))
        np.testing.assert_allclose(e32[:w], e64[:w], rtol=1e-5)
        assert np.linalg.norm(f - Ah @ y32) <= 10 * max(np.linalg.norm(f - Ah @ y64), 1e-13 * np.linalg.norm(f))

    preS = hipla.DiagonalMatrix(1.0 / s.mass)
    Km = hipla.BlockMatrix([[A, B.T], [B, None]])
    counts = {"minres": 0}
    orig = fused.MinresLoop.run

    def counting(self, *a, **kw):
        counts["minres"] += 1
        return orig(self, *a, **kw)
    out = {}
    fused.MinresLoop.run = counting
    try:
        for st in ("fp64", "fp32"):
            Cm = hipla.BlockMatrix([[hipla.SmoothedAggregationAMG(A, storage=st), None], [None, preS]])
            with contextlib.redirect_stdout(io.StringIO()):
                out[st] = MinRes(mat=Km, pre=Cm, rhs=hipla.BlockVector([fv, hipla.Vector.from_numpy(g)]),
                                 maxsteps=3000, tol=1e-9, printrates=False)
    finally:
        fused.MinresLoop.run = orig
    assert counts["minres"] == 2
    e64, e32 = np.asarray(out["fp64"][1]), np.asarray(out["fp32"][1])
    assert abs(len(e32) - len(e64)) <= max(3, int(0.03 * len(e64)))
    w = min(20, len(e64), len(e32))
    np.testing.assert_allclose(e32[:w], e64[:w], rtol=1e-5)
