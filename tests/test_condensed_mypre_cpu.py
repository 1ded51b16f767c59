"""The reference's default Stokes solve, SolveInitial(iterative=True) (templates/NavierStokesSIMPLE_iterative.py:188,
364-397): a statically condensed blfA and the multiplicative MypreA (GS=True) over its Schur complement, with blocks
of coupling dofs only.  Host logic on the numpy checker engine: the driver against the oracle, the decline reasons of
the fused loop, the sizes the C ABI checks."""
import contextlib
import io
import re

import numpy as np
import pytest

from oracle import krylov_ref as kr


@contextlib.contextmanager
def sessions_recorded():
    """The BpcgSession objects BramblePasciakCG builds, in order (k, fused, fused_declined, lanczos_native)."""
    import solvers.bramblepasciak_new as bp
    made = []
    orig = bp.BpcgSession

    class Recording(orig):
        def __init__(self, *a, **kw):
            super().__init__(*a, **kw)
            made.append(self)
    bp.BpcgSession = Recording
    try:
        yield made
    finally:
        bp.BpcgSession = orig


def _history(text):
    return np.array([float(m) for m in re.findall(r"it =\s+\d+\s+err =\s+(\S+)", text)])


@pytest.mark.parametrize("dim,maxh", [(2, 1.0 / 8), (3, 1.0 / 5)])
def test_solve_initial_condensed_against_oracle(numpy_engine, dim, maxh):
    """SolveInitial(condense=True) = kr.bpcg_v2 on the Schur complement with kr.mypre_a(S, blocks, aux, gs=True) and
    the condensed branch of harmonic_extension, in the same block order, with the same k; the blocks hold coupling
    dofs only (padding last, empty blocks dropped)."""
    import hipla
    from templates.NavierStokesSIMPLE_iterative import NavierStokes, SyntheticMesh
    ns = NavierStokes(SyntheticMesh(maxh, dim=dim), nu=0.01, inflow="inlet", outflow="outlet", wall="wall|cyl",
                      uin=None, timestep=0.001, order=1)
    tol, maxsteps = 1e-8, 3000
    out = io.StringIO()
    with contextlib.redirect_stdout(out), sessions_recorded() as made:
        ns.SolveInitial(iterative=True, GS=True, tol=tol, maxsteps=maxsteps, printrates=True, condense=True)
    ses, = made
    assert ses.blfA.condense
    assert ses.fused is None and ses.fused_declined == "not the HIP engine"
    s = ns.system
    parts = s.condense()
    interior = parts["interior"]
    preA = ns.preA
    assert preA.mat is ses.blfA.mat                                   # the sweeps run over S
    idx = preA.idx_host
    assert not np.isin(idx[idx >= 0], np.nonzero(interior)[0]).any()  # coupling dofs only
    assert (idx >= 0).any(axis=0).all()                               # no empty block
    live = idx >= 0
    assert not (~live[:-1] & live[1:]).any()                          # padding last
    assert np.array_equal(np.sort(idx[live]), np.nonzero(~interior)[0])   # every coupling dof in one block

    aux = preA.middle

    def aux_apply(r):
        y = hipla.Vector(s.n_u)
        aux.Mult(hipla.Vector.from_numpy(r), y)
        return y.numpy()

    S = parts["mat"]
    pa = kr.mypre_a(S, idx, aux_apply, gs=True)
    # the scale factor of a Lanczos stopped at tol=1e-3 (Ritz values not converged, orthogonality lost): the block
    # solves of the engine (inverse blocks) and of the oracle (LAPACK) round differently, which moves the smallest
    # Ritz value by ~1e-7 here; the solve below uses the session's k
    k = kr.scale_factor(kr.lanczos_ritz(s.A, pa, tol=1e-3))
    assert abs(k - ses.k) < 1e-6 * k
    f, g = ns.f.vec.numpy(), ns.g.vec.numpy()
    mass = ns.mp.mat.to_scipy().diagonal()
    condensed = {key: parts[key] for key in ("harmonic_extension", "harmonic_extension_trans", "inner_solve",
                                             "inner_matrix")}
    it_ref, u_ref, p_ref, hist_ref, _ = kr.bpcg_v2(S, s.B, pa, kr.diag_inverse(mass), f, g, ses.k, tol=tol,
                                                   maxsteps=maxsteps, condensed=condensed)
    hist = _history(out.getvalue())
    w = min(20, len(hist), len(hist_ref))
    np.testing.assert_allclose(hist[:w], hist_ref[:w], rtol=1e-8)
    it = ns.stokes_bpcg_iterations
    assert abs(it - it_ref) <= max(3, int(0.05 * it_ref))
    x, x_ref = np.concatenate([ns.gfu.numpy(), ns.gfup.numpy()]), np.concatenate([u_ref, p_ref])
    assert np.linalg.norm(x - x_ref) < 1e-5 * np.linalg.norm(x_ref)
    assert 3 < it < maxsteps


def test_solve_initial_condense_keyword(numpy_engine):
    """The default stays uncondensed; amg=True does not combine with condense=True."""
    from templates.NavierStokesSIMPLE_iterative import NavierStokes, SyntheticMesh
    ns = NavierStokes(SyntheticMesh(1.0 / 6, dim=2), nu=0.01, inflow="inlet", outflow="outlet", wall="wall|cyl",
                      uin=None, timestep=0.001, order=1)
    with contextlib.redirect_stdout(io.StringIO()), sessions_recorded() as made:
        ns.SolveInitial(iterative=True, tol=1e-8)
    assert not made[0].blfA.condense and ns.preA.mat is ns.a.mat
    with pytest.raises(ValueError, match="condense"):
        ns.SolveInitial(iterative=True, amg=True, condense=True)


def test_coupling_blocks():
    from templates.NavierStokesSIMPLE_iterative import coupling_blocks
    blocks = np.array([[0, 3, 6, 9], [1, 4, 7, -1], [2, 5, -1, -1]], dtype=np.int32)
    interior = np.zeros(10, dtype=bool)
    interior[[0, 3, 4, 5, 7]] = True
    got = coupling_blocks(blocks, interior)
    assert got.dtype == np.int32 and got.flags.c_contiguous
    np.testing.assert_array_equal(got, [[1, 6, 9], [2, -1, -1], [-1, -1, -1]])    # (the order inside a block kept)


def _condensed_operands(dim=2, n=6):
    import hipla
    from discretizations import CondensedForm
    from staggered_grid import mac_stokes
    from templates.NavierStokesSIMPLE_iterative import MypreA, auxiliary_space_preconditioner, coupling_blocks
    s = mac_stokes(dim, n, 0.01)
    blfA = CondensedForm(s)
    _, _, aux = auxiliary_space_preconditioner(s)
    preA = MypreA(None, blfA, coupling_blocks(s.facet_blocks(), blfA.interior), GS=True, aux=aux)
    B = hipla.SparseMatrix.from_scipy(s.B)
    vecs = {name: hipla.Vector(s.n_u) for name in ("u0", "d0", "w0", "s0", "z0", "q", "t0", "t1", "t2", "t4")}
    vecs.update({name: hipla.Vector(s.n_p) for name in ("u1", "d1", "w1", "s1", "t3")})
    explicit = hipla.SparseMatrix.from_scipy(s.A)
    condensed = dict(HT=blfA.harmonic_extension_trans, H=blfA.harmonic_extension, inner=blfA.inner_solve, S=blfA.mat)
    return s, blfA, preA, B, explicit, vecs, condensed


def test_fused_declined_reasons(numpy_engine, monkeypatch):
    """Bpcg2Loop.try_create says why it returns None -- here past the engine check, so that the reasons of the
    combinations still declined show: condensed on a partitioned run, a multiplicative MypreA that does not sweep over
    the Schur complement, and (BpcgSession) a given matC.  MinresLoop, Bpcg1Loop and CgLoop keep theirs the same
    way."""
    import hipla
    from hipla import fused
    from solvers.bramblepasciak_new import BpcgSession
    s, blfA, preA, B, explicit, vecs, condensed = _condensed_operands()
    preM = hipla.DiagonalMatrix(1.0 / s.mass)
    BT = B.CreateTranspose()
    monkeypatch.setattr(fused, "_hip", lambda eng: True)
    Loop = fused.Bpcg2Loop
    assert Loop.try_create(explicit, B, BT, preA, 1.0, preM, vecs, distributed=True, condensed=condensed) is None
    assert "partitioned" in Loop.last_declined
    assert Loop.try_create(explicit, B, BT, blfA.jacobi(), 1.0, preM, vecs, distributed=True,
                           condensed=condensed) is None
    assert Loop.last_declined == "condensed form on a partitioned run"
    no_s = {key: val for key, val in condensed.items() if key != "S"}
    assert Loop.try_create(explicit, B, BT, preA, 1.0, preM, vecs, condensed=no_s) is None
    assert "Schur complement" in Loop.last_declined
    other = dict(condensed, S=hipla.SparseMatrix.from_scipy(s.condense()["mat"]))
    assert Loop.try_create(explicit, B, BT, preA, 1.0, preM, vecs, condensed=other) is None
    assert "Schur complement" in Loop.last_declined
    assert Loop.try_create(explicit, B, BT, preA, 1.0, preA, vecs, condensed=condensed) is None
    assert Loop.last_declined == "preM is not a (scaled) diagonal"
    bad = dict(vecs, t2=hipla.Vector(s.n_u + 1))
    assert Loop.try_create(explicit, B, BT, preA, 1.0, preM, bad, condensed=condensed) is None
    assert "work vector" in Loop.last_declined

    # MINRES, BPCG v1 and CG say why as well
    M, Bp1, Cg = fused.MinresLoop, fused.Bpcg1Loop, fused.CgLoop
    A, bjac = explicit, hipla.BlockJacobi(explicit, s.line_blocks(3))
    K = hipla.BlockMatrix([[A, BT], [B, None]])

    def block(n_p=s.n_p):
        return hipla.BlockVector([hipla.Vector(s.n_u), hipla.Vector(n_p)])

    def minres(pre_a, pre_s=preM, mat=K, u=None):
        return M.try_create(mat, hipla.BlockMatrix([[pre_a, None], [None, pre_s]]), u or block(),
                            [block() for _ in range(3)], [block() for _ in range(3)], [block() for _ in range(2)], block())

    assert minres(2.0 * bjac) is None and M.last_declined == "preA is not native"
    assert minres(preA) is None and M.last_declined == "preA is not native"
    assert minres(bjac, pre_s=bjac) is None and M.last_declined == "preS is not a (scaled) diagonal"
    assert minres(bjac, mat=hipla.BlockMatrix([[A, BT], [B, A]])) is None
    assert M.last_declined == "K or C has another non-zero block"
    assert minres(bjac, u=block(s.n_p + 1)) is None and "work vector" in M.last_declined
    pair = {name: block() for name in ("x", "r", "d", "a", "t1", "t2")}
    assert Bp1.try_create(A, B, A, bjac, preM, 1.0, pair) is None and Bp1.last_declined == "C is given"
    assert Bp1.try_create(A, B, None, preA, preM, 1.0, pair) is None and Bp1.last_declined == "preA is not native"
    assert Bp1.try_create(A, B, None, bjac, bjac, 1.0, pair) is None
    assert Bp1.last_declined == "preS is not a (scaled) diagonal"
    assert Bp1.try_create(A, B, None, bjac, preM, 1.0, dict(pair, t2=hipla.Vector(s.n_u))) is None
    assert "work vector" in Bp1.last_declined
    assert Cg.try_create(B, None) is None and Cg.last_declined == "the matrix is not a square SparseMatrix"
    assert Cg.try_create(A, 2.0 * bjac) is None and Cg.last_declined == "the preconditioner is scaled or a sum"
    assert Cg.try_create(A, preA) is None and Cg.last_declined == "the preconditioner is not native"

    monkeypatch.setattr(fused, "ENABLED", False)
    assert Loop.try_create(explicit, B, BT, preA, 1.0, preM, vecs, condensed=condensed) is None
    assert "ENABLED" in Loop.last_declined
    assert minres(bjac) is None and "ENABLED" in M.last_declined
    assert Bp1.try_create(A, B, None, bjac, preM, 1.0, pair) is None and "ENABLED" in Bp1.last_declined
    assert Cg.try_create(A, None) is None and "ENABLED" in Cg.last_declined
    monkeypatch.undo()
    assert Cg.try_create(A, bjac) is None and Cg.last_declined == "not the HIP engine"

    from discretizations import AssembledForm
    f, g = s.rhs(0)
    with contextlib.redirect_stdout(io.StringIO()):
        ses = BpcgSession(blfA, AssembledForm(B), object(), hipla.Vector.from_numpy(f), hipla.Vector.from_numpy(g),
                          preA, preM, k=1.5)
    assert ses.fused is None and "matC" in ses.fused_declined
    assert ses.lanczos_native is False


def test_native_lanczos_declines_on_the_checker_engine(numpy_engine):
    """`info` reports the device-resident Lanczos; off the HIP engine the protocol recurrence runs on the explicit
    product with MypreA over S and gives the oracle's Ritz values."""
    import hipla
    from hipla.eigen import EigenValues_Preconditioner
    s, blfA, preA, B, explicit, vecs, condensed = _condensed_operands()
    info = {}
    with contextlib.redirect_stdout(io.StringIO()):
        lams = EigenValues_Preconditioner(explicit, preA, tol=1e-3, sweep_A=blfA.mat, info=info)
    assert info == {"native": False}

    def aux_apply(r):
        y = hipla.Vector(s.n_u)
        preA.middle.Mult(hipla.Vector.from_numpy(r), y)
        return y.numpy()
    ref = kr.lanczos_ritz(s.A, kr.mypre_a(s.condense()["mat"], preA.idx_host, aux_apply, gs=True), tol=1e-3)
    # a Lanczos stopped at tol=1e-3 has lost orthogonality: the rounding of the block solves (inverse blocks here,
    # LAPACK in the oracle) moves its interior Ritz values by percents and the smallest one by ~1e-6
    assert abs(min(lams) - min(ref)) < 1e-5 * abs(min(ref))
    assert abs(max(lams) - max(ref)) < 1e-5 * abs(max(ref))


def test_state_mirrors_end_with_sweep_A():
    """nss_bpcg2_t and nss_lanczos_t gained one field, appended: sweep_A (NULL = the loop's own A)."""
    from hipla import eigen, fused
    assert fused.Bpcg2State._fields_[-1][0] == "sweep_A"
    assert eigen._LanczosState.get()._fields_[-1][0] == "sweep_A"
    with open(__import__("conftest").ROOT + "/include/nss_krylov.h") as fh:
        header = fh.read()
    for struct in ("nss_bpcg2_t", "nss_lanczos_t"):
        body = header[:header.index("} %s;" % struct)]
        assert body.rstrip().endswith("nss_csr_t sweep_A;"), struct


def test_condensed_fusable_structure(numpy_engine):
    """The structural checks of the fused condensed forms (hipla.fused.condensed_fusable) accept the grid's operators
    and reject hand-built matrices that break each assumption; a sweep outside the colour-major layout is declined."""
    import types

    import hipla
    from hipla import fused
    s, blfA, preA, B, explicit, vecs, condensed = _condensed_operands()
    sweep = types.SimpleNamespace(layout="colour-major", mat=blfA.mat, n=s.n_u, idx_host=preA.idx_host,
                                  engine=preA.engine)
    assert fused.condensed_fusable(sweep, condensed) == (True, None)
    assert not fused.condensed_fusable(types.SimpleNamespace(**dict(vars(sweep), layout="rows")), condensed)[0]
    interior = np.nonzero(blfA.interior)[0]
    coupling = np.nonzero(~blfA.interior)[0]
    i, c = int(interior[0]), int(coupling[0])

    def plus(key, row, col, val=1.0):
        m = condensed[key].to_scipy().tolil()
        m[row, col] = m[row, col] + val
        return dict(condensed, **{key: hipla.SparseMatrix.from_scipy(m.tocsr())})

    cases = {"H^T has rows outside": plus("HT", i, c),
             "S has entries outside": plus("S", c, i),
             "A_ii^-1 is not diagonal": plus("inner", i, int(interior[1])),
             "A_ii^-1 is not diagonal outside": plus("inner", c, c),
             "H does not map": plus("H", c, c)}
    bad_col = condensed["H"].to_scipy().tolil()
    bad_col[i, int(interior[1])] = 1.0
    cases["H does not map "] = dict(condensed, H=hipla.SparseMatrix.from_scipy(bad_col.tocsr()))
    for want, cond in cases.items():
        if "S has" in want:
            sweep_s = types.SimpleNamespace(**dict(vars(sweep), mat=cond["S"]))
            ok, why = fused.condensed_fusable(sweep_s, cond)
        else:
            ok, why = fused.condensed_fusable(sweep, cond)
        assert not ok and why.startswith(want.strip().split(" outside")[0]), (want, why)
    full = types.SimpleNamespace(**dict(vars(sweep), idx_host=np.arange(s.n_u, dtype=np.int32)[None, :]))
    assert fused.condensed_fusable(full, condensed) == (False, "every dof is in a block")
