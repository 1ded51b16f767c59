"""The reference's default Stokes solve on the MI355X: a statically condensed blfA (templates/
NavierStokesSIMPLE_iterative.py:188) with the multiplicative MypreA (GS=True, :364-391) over its Schur complement S,
blocks of coupling dofs only.  The fused BPCG v2 loop and the device-resident Lanczos take it (nss_bpcg2_t.sweep_A,
nss_lanczos_t.sweep_A = S); checked against the oracle and against the statement-by-statement protocol path."""
import contextlib
import io
import re

import numpy as np
import pytest

from oracle import krylov_ref as kr
from staggered_grid import mac_stokes

pytestmark = pytest.mark.gpu


class Form:
    def __init__(self, mat):
        self.mat, self.condense = mat, False


@contextlib.contextmanager
def bpcg2_runs_counted():
    from hipla import fused
    counts = [0]
    orig = fused.Bpcg2Loop.run

    def counting(self, *a, **kw):
        counts[0] += 1
        return orig(self, *a, **kw)
    fused.Bpcg2Loop.run = counting
    try:
        yield counts
    finally:
        fused.Bpcg2Loop.run = orig


def _history(text):
    return np.array([float(m) for m in re.findall(r"it =\s+\d+\s+err =\s+(\S+)", text)])


def _operands(s):
    import hipla
    from discretizations import CondensedForm
    from templates.NavierStokesSIMPLE_iterative import MypreA, auxiliary_space_preconditioner, coupling_blocks
    blfA = CondensedForm(s)
    _, _, aux = auxiliary_space_preconditioner(s)
    preA = MypreA(None, blfA, coupling_blocks(s.facet_blocks(), blfA.interior), GS=True, aux=aux)
    return blfA, Form(hipla.SparseMatrix.from_scipy(s.B)), preA, hipla.DiagonalMatrix(1.0 / s.mass)


def _solve(s, blfA, blfB, preA, preM, tol, maxsteps):
    import hipla
    from solvers.bramblepasciak_new import BramblePasciakCG
    f, g = s.rhs(0)
    sol = hipla.BlockVector([hipla.Vector(s.n_u), hipla.Vector(s.n_p)])
    out = io.StringIO()
    with contextlib.redirect_stdout(out), bpcg2_runs_counted() as runs:
        it, _ = BramblePasciakCG(blfA, blfB, None, hipla.Vector.from_numpy(f), hipla.Vector.from_numpy(g), preA, preM,
                                 sol, tol=tol, maxsteps=maxsteps)
    return it, _history(out.getvalue()), sol.numpy(), runs[0]


# history windows: the functional sqrt|<w, d>| of the condensed 2-D case cancels from entry 12 on (two entries there
# differ by 5.7e-5 between GPU and oracle, measured; the first 12 agree to 1e-8)
@pytest.mark.parametrize("dim,n,window", [(2, 16, 12), (3, 8, 20)])
def test_condensed_multiplicative_mypre_a_fused(hip_engine, dim, n, window):
    """The fused loop and the native Lanczos run; k, history, iteration count, solution and true saddle residual
    against kr.bpcg_v2(..., condensed=...) with kr.mypre_a(S, blocks, aux, gs=True) in the GPU's colour-major block
    order (the GPU's auxiliary term as a black box), and against the protocol path (fused.ENABLED = False)."""
    import hipla
    from hipla import fused
    from solvers.bramblepasciak_new import BpcgSession
    s = mac_stokes(dim, n, 0.01)
    f, g = s.rhs(0)
    blfA, blfB, preA, preM = _operands(s)
    assert preA.n_uncovered == int(blfA.interior.sum()) > 0        # every interior dof is outside the blocks
    tol, maxsteps = 1e-9, 3000
    with contextlib.redirect_stdout(io.StringIO()):
        ses = BpcgSession(blfA, blfB, None, hipla.Vector.from_numpy(f), hipla.Vector.from_numpy(g), preA, preM)
    assert ses.fused is not None, ses.fused_declined
    assert ses.fused_declined is None and ses.lanczos_native
    assert ses.fused.state.sweep_A == blfA.mat.handle.ptr.value

    parts = s.condense()
    S = parts["mat"]

    def aux_apply(r):
        y = hipla.Vector(s.n_u)
        preA.middle.Mult(hipla.Vector.from_numpy(r), y)
        return y.numpy()
    pa, ps = kr.mypre_a(S, preA.idx_host, aux_apply, gs=True), kr.diag_inverse(s.mass)
    # a Lanczos stopped at tol=1e-3 has lost orthogonality: the rounding of the block solves (packed inverses on the
    # GPU, LAPACK in the oracle) moves the smallest Ritz value by ~1e-7 .. 1e-6 (measured on the checker engine)
    k = kr.scale_factor(kr.lanczos_ritz(s.A, pa, tol=1e-3))
    assert abs(k - ses.k) < 1e-5 * k

    it, hist, x, runs = _solve(s, blfA, blfB, preA, preM, tol, maxsteps)
    assert runs == 1, "the fused device loop did not run"
    condensed = {key: parts[key] for key in ("harmonic_extension", "harmonic_extension_trans", "inner_solve",
                                             "inner_matrix")}
    it_ref, u_ref, p_ref, hist_ref, _ = kr.bpcg_v2(S, s.B, pa, ps, f, g, ses.k, tol=tol, maxsteps=maxsteps,
                                                   condensed=condensed)
    w = min(window, len(hist), len(hist_ref))
    np.testing.assert_allclose(hist[:w], hist_ref[:w], rtol=1e-8)
    assert abs(it - it_ref) <= max(3, int(0.05 * it_ref))
    x_ref = np.concatenate([u_ref, p_ref])
    assert np.linalg.norm(x - x_ref) < 1e-5 * np.linalg.norm(x_ref)
    b, K = np.concatenate([f, g]), s.saddle_matrix()
    r, r_ref = np.linalg.norm(b - K @ x), np.linalg.norm(b - K @ x_ref)
    assert abs(r - r_ref) < 1e-3 * r_ref + 1e-6 * np.linalg.norm(b)
    assert 3 < it < maxsteps

    # the protocol path: its own Lanczos (protocol recurrence) gives k to the same ~1e-6; the loop is compared with
    # the fused one's k, as the oracle is
    fused.ENABLED = False
    try:
        with contextlib.redirect_stdout(io.StringIO()):
            ses_p = BpcgSession(blfA, blfB, None, hipla.Vector.from_numpy(f), hipla.Vector.from_numpy(g), preA, preM)
        assert ses_p.fused is None and not ses_p.lanczos_native
        assert abs(ses_p.k - ses.k) < 1e-5 * ses.k
        sol = hipla.BlockVector([hipla.Vector(s.n_u), hipla.Vector(s.n_p)])
        out = io.StringIO()
        with contextlib.redirect_stdout(out):
            ses_p = BpcgSession(blfA, blfB, None, hipla.Vector.from_numpy(f), hipla.Vector.from_numpy(g), preA, preM,
                                sol=sol, k=ses.k)
            assert ses_p.fused is None
            it_p, _ = ses_p.protocol_loop(tol, maxsteps, True, True)    # what BramblePasciakCG runs without a loop
    finally:
        fused.ENABLED = True
    hist_p, x_p = _history(out.getvalue()), sol.numpy()
    w = min(window, len(hist), len(hist_p))
    np.testing.assert_allclose(hist[:w], hist_p[:w], rtol=1e-8)
    assert abs(it - it_p) <= max(3, int(0.05 * it_p))
    assert np.linalg.norm(x - x_p) < 1e-5 * np.linalg.norm(x_p)


def test_solve_initial_condensed_takes_the_fused_loop(hip_engine):
    """NavierStokes.SolveInitial(condense=True) on a 3-D mesh: the fused loop runs, and velocity and pressure agree with
    SolveInitial(condense=False) to the solver tolerance -- both solve the same saddle system."""
    from templates.NavierStokesSIMPLE_iterative import NavierStokes, SyntheticMesh
    res = {}
    for condense in (False, True):
        ns = NavierStokes(SyntheticMesh(1.0 / 8, dim=3), nu=0.01, inflow="inlet", outflow="outlet", wall="wall|cyl",
                          uin=None, timestep=0.001, order=1)
        with contextlib.redirect_stdout(io.StringIO()), bpcg2_runs_counted() as runs:
            ns.SolveInitial(iterative=True, GS=True, tol=1e-10, condense=condense)
        assert runs[0] == 1, condense
        res[condense] = (ns.gfu.numpy(), ns.gfup.numpy(), ns.stokes_bpcg_iterations, ns.system)
    (u0, p0, it0, s), (u1, p1, it1, _) = res[False], res[True]
    assert np.linalg.norm(u1 - u0) < 1e-6 * np.linalg.norm(u0)
    assert np.linalg.norm(p1 - p0) < 1e-6 * np.linalg.norm(p0)
    f, g = s.rhs(0)
    b = np.concatenate([f, g])
    assert np.linalg.norm(b - s.saddle_matrix() @ np.concatenate([u1, p1])) < 1e-6 * np.linalg.norm(b)
    assert 3 < it1 < 100000 and 3 < it0 < 100000


@pytest.mark.parametrize("dim,n", [(2, 16), (3, 8)])
def test_condensed_fused_forms_against_straightforward_sequence(hip_engine, dim, n):
    """NSS_COND_FUSE on and off (nss_cond_fuse_mode): the fused condensed forms are attached for the grid's operators,
    one preconditioner apply (K1 of iteration 0: t1 = harmonic_extension around MypreA) agrees to 1e-13 relative with
    the straightforward sequence, and the solves need the same iterations (to one)."""
    import hipla
    from solvers.bramblepasciak_new import BpcgSession
    s = mac_stokes(dim, n, 0.01)
    f, g = s.rhs(0)
    blfA, blfB, preA, preM = _operands(s)
    applies, counts = {}, {}
    for mode in (1, 0):
        with hip_engine.overrides(cond_fuse=mode):
            with contextlib.redirect_stdout(io.StringIO()):
                ses = BpcgSession(blfA, blfB, None, hipla.Vector.from_numpy(f), hipla.Vector.from_numpy(g), preA,
                                  preM, k=1.7)
            assert ses.fused is not None and ses.fused.cond_fusable, ses.fused.cond_fuse_declined
            ses.first_direction()
            ses.fused.start(ses.wdn, ses.err0, 1e-9, True, 10)
            ses.fused.phase("K1", 0)
            hip_engine.synchronize()
            applies[mode] = ses.t1.numpy().copy()
            it, _, _, runs = _solve(s, blfA, blfB, preA, preM, 1e-9, 3000)
            assert runs == 1
            counts[mode] = it
    scale = np.abs(applies[0]).max()
    assert scale > 0
    assert np.abs(applies[1] - applies[0]).max() <= 1e-13 * scale
    # the forms agree to rounding, not bitwise: the stop test of a ~200-iteration solve may fire one iteration apart
    # (measured: 193 against 194 at 2-D n = 16, the same count at 3-D n = 8)
    assert abs(counts[1] - counts[0]) <= 1
