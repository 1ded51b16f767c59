"""Launch plans of matrices shared between consumers.

A re-plan (nss_csr_plan_for_pairs, nss_csr_plan_for_blocks, the joint cycle of nss_amg_create_auxiliary) rewrites a
matrix in place and changes its row-block count, hence the number of dot partials every fused loop over it writes and
sums.  A loop that sized its partials before such a re-plan must not launch with them: the library refuses the stale
state (its `plan_gen` no longer matches nss_csr_plan_generation), and the host loop objects re-size before their next
run.  Each scenario shows the stale sizes on the host (workspace query only, nothing launched), that the library
refuses the stale state, and that the loop afterwards computes what a loop built after the re-plan computes -- bit for
bit -- within the oracle contract of tests/test_hip_solvers.py."""

import contextlib
import ctypes as C
import io

import numpy as np
import pytest

from oracle import krylov_ref as kr
from staggered_grid import mac_stokes

pytestmark = pytest.mark.gpu


class Form:
    def __init__(self, mat):
        self.mat, self.condense = mat, False


def require_guard(eng):
    """Never drive a stale state into a library without the guard: it would write past its partials buffers."""
    from hipla import eigen, fused
    if not hasattr(eng.lib, "nss_csr_plan_generation"):
        pytest.fail("the library has no plan-generation guard (nss_csr_plan_generation)")
    for st in (fused.Bpcg2State, fused.MinresState, fused.Bpcg1State, fused.CgState, eigen._LanczosState.get()):
        if "plan_gen" not in [name for name, _ in st._fields_]:
            pytest.fail("%s has no plan_gen field" % st.__name__)


def workspace(fn, st, n):
    out = [C.c_int64() for _ in range(n)]
    assert fn(C.byref(st), *(C.byref(o) for o in out)) == 0
    return [o.value for o in out]


def caps(st, n):
    return [st.cap_a, st.cap_b, st.cap_c][:n]


# block-structured (inflated) systems first: ~25 non-zeros per row, so that a re-plan moves the row-block counts
CANDIDATES = ((2, 12, 5), (2, 16, 5), (3, 5, 4), (2, 24, 1), (3, 6, 1))


def stale(eng, st, mats):
    """The state's recorded plan generation is behind its matrices (checked on the host before the library is asked
    to refuse it: a state whose generation did not move is never handed to a launching entry point here)."""
    from hipla import fused
    return st.plan_gen != fused.plan_stamp(eng, *(getattr(st, m) for m in mats))


def assert_refused(eng, call, st, mats, keep):
    """The launching entry point refuses the stale state.  `keep`: buffers the host sets only when a solve starts
    (history, iterate), given to the state so that the plan guard -- not a NULL check -- is what refuses."""
    assert stale(eng, st, mats)
    for name, buf in keep.items():
        setattr(st, name, buf.data_ptr())
    rc = call(C.byref(st))
    assert rc != 0
    assert b"re-planned" in eng.lib.nss_last_error(), eng.lib.nss_last_error()


def system(dim, n, inflate=1):
    import hipla
    s = mac_stokes(dim, n, 0.01)
    if inflate > 1:
        s = s.inflate(inflate)
    f, g = s.rhs(0)
    A, B = hipla.SparseMatrix.from_scipy(s.A), hipla.SparseMatrix.from_scipy(s.B)
    return s, f, g, A, B


def session(A, B, f, g, preA, preS, k=None):
    import hipla
    from solvers.bramblepasciak_new import BpcgSession
    with contextlib.redirect_stdout(io.StringIO()):
        ses = BpcgSession(Form(A), Form(B), None, hipla.Vector.from_numpy(f), hipla.Vector.from_numpy(g), preA, preS,
                          k=k)
    assert ses.fused is not None
    return ses


def solve(ses, tol=1e-9, maxsteps=2000):
    """The loop of BramblePasciakCG on a session built before: (it, history, solution)."""
    ses.first_direction()
    it, hist, done = ses.fused.run(ses.wdn, ses.err0, tol, True, maxsteps)
    assert done
    return it, np.asarray(hist), np.concatenate([ses.u[0].numpy(), ses.u[1].numpy()])


def check_against_bpcg_v2(s, f, g, pa, k, it, hist, x, tol=1e-9):
    it_ref, u, p, hist_ref, _ = kr.bpcg_v2(s.A, s.B, pa, kr.diag_inverse(s.mass), f, g, k, tol=tol, maxsteps=2000)
    w = min(20, len(hist), len(hist_ref))
    np.testing.assert_allclose(hist[:w], hist_ref[:w], rtol=1e-8)
    assert abs(it - it_ref) <= max(3, int(0.03 * it_ref + 0.999))
    x_ref = np.concatenate([u, p])
    assert np.linalg.norm(x - x_ref) < 1e-5 * np.linalg.norm(x_ref)


def test_bpcg_session_after_bramble_pasciak_cg_with_block_jacobi(hip_engine):
    """A BpcgSession (fused BPCG v2, point-Jacobi preA) is built; bramble_pasciak_cg with block Jacobi then re-plans
    the SAME A around its blocks (bramble_pasciak_cg.py: plan_for_textbook_bpcg, and the Bpcg1Loop); then the session
    solves.  Its loop re-sizes and agrees bit for bit with a session built after the re-plan (same k).  Block-structured
    (inflated) systems: ~25 non-zeros per row and 15-dof blocks, so that row blocks starting at block starts are
    more (on the plain grid the plan around line blocks happens to keep A's row-block count)."""
    import hipla
    from bramble_pasciak_cg import bramble_pasciak_cg
    eng = hip_engine
    require_guard(eng)
    for dim, n, inflate in ((2, 12, 5), (2, 16, 5), (3, 5, 4), (2, 24, 1)):
        s, f, g, A, B = system(dim, n, inflate)
        preA, preS = hipla.JacobiPreconditioner(A), hipla.DiagonalMatrix(1.0 / s.mass)
        ses = session(A, B, f, g, preA, preS)
        st = ses.fused.state
        before = workspace(eng.lib.nss_bpcg2_workspace, st, 3)
        assert before == caps(st, 3)
        gen, nblk = A.handle.plan_generation(), A.handle.info()["row_blocks"]
        with contextlib.redirect_stdout(io.StringIO()):
            bramble_pasciak_cg(A, B, None, hipla.BlockJacobi(A, s.line_blocks(3)), preS, hipla.Vector.from_numpy(f),
                               hipla.Vector.from_numpy(g), tolerance=1e-9, max_steps=2000, print_rates=False)
        assert A.handle.plan_generation() > gen
        after = workspace(eng.lib.nss_bpcg2_workspace, st, 3)
        if A.handle.info()["row_blocks"] != nblk:
            break
    else:
        pytest.fail("no system size where block Jacobi re-plans A to another row-block count")
    assert after != caps(st, 3), (after, caps(st, 3))           # the stale sizes, shown on the host
    assert_refused(eng, lambda p: eng.lib.nss_bpcg2_iterate(p, 0, 1, eng.stream), st, ("A", "B", "BT"),
                   {"hist": eng.zeros(4)})
    it, hist, x = solve(ses)
    assert caps(st, 3) == [max(1, v) for v in after] and st.plan_gen == A.handle.plan_generation()
    it2, hist2, x2 = solve(session(A, B, f, g, preA, preS, k=ses.k))
    assert it == it2
    np.testing.assert_array_equal(hist, hist2)
    np.testing.assert_array_equal(x, x2)
    check_against_bpcg_v2(s, f, g, kr.jacobi(s.A), ses.k, it, hist, x)


def test_bpcg2_and_bpcg1_with_different_block_jacobi_handles(hip_engine):
    """Bpcg2Loop with block Jacobi J1 plans B^T around J1 (fused.py: c1_applies_bjac) and pair-plans B; a Bpcg1Loop
    built before on the same B (its B^T is the same cached transpose) is then stale, and bramble_pasciak_cg with
    another handle J3 re-plans A under the Bpcg2Loop.  Each loop refuses while stale and re-sizes."""
    import hipla
    from bramble_pasciak_cg import bramble_pasciak_cg
    from hipla import fused
    eng = hip_engine
    require_guard(eng)
    seen = []
    for dim, n, inflate in CANDIDATES:
        s, f, g, A, B = system(dim, n, inflate)
        preS = hipla.DiagonalMatrix(1.0 / s.mass)
        blocks = s.line_blocks(3 if inflate == 1 else 1)
        J1, J2, J3 = (hipla.BlockJacobi(A, blocks) for _ in range(3))      # three handles, the same blocks
        zero2 = lambda: hipla.BlockVector([hipla.Vector(s.n_u), hipla.Vector(s.n_p)])
        loop1 = fused.Bpcg1Loop.try_create(A, B, None, J2, preS, 1.0,
                                           {name: zero2() for name in ("x", "r", "d", "a", "t1", "t2")})
        assert loop1 is not None
        st1 = loop1.state
        assert workspace(eng.lib.nss_bpcg1_workspace, st1, 3) == caps(st1, 3)
        nblk_b, gen_b = B.handle.info()["row_blocks"], B.handle.plan_generation()
        ses = session(A, B, f, g, J1, preS)                      # Bpcg2Loop: plan_for_pairs(B), plan_for_blocks(B^T, J1)
        seen.append((dim, n, inflate, nblk_b, B.handle.info()["row_blocks"], gen_b, B.handle.plan_generation()))
        if B.handle.info()["row_blocks"] != nblk_b:
            break
    else:
        pytest.fail("no system size where the pair-plan moves B's row-block count: %r" % (seen,))
    assert workspace(eng.lib.nss_bpcg1_workspace, st1, 3) != caps(st1, 3)
    assert_refused(eng, lambda p: eng.lib.nss_bpcg1_iterate(p, 0, 1, eng.stream), st1, ("A", "B", "BT"),
                   {"hist": eng.zeros(4)})
    loop1.partials = fused.fit_partials(eng, st1, eng.lib.nss_bpcg1_workspace, ("A", "B", "BT"), loop1.partials)
    assert workspace(eng.lib.nss_bpcg1_workspace, st1, 3) == caps(st1, 3)
    # bramble_pasciak_cg with J3 re-plans A (plan_for_textbook_bpcg, Bpcg1Loop) under the session's loop
    st2 = ses.fused.state
    gen = A.handle.plan_generation()
    with contextlib.redirect_stdout(io.StringIO()):
        bramble_pasciak_cg(A, B, None, J3, preS, hipla.Vector.from_numpy(f), hipla.Vector.from_numpy(g),
                           tolerance=1e-9, max_steps=2000, print_rates=False)
    assert A.handle.plan_generation() > gen
    assert_refused(eng, lambda p: eng.lib.nss_bpcg2_iterate(p, 0, 1, eng.stream), st2, ("A", "B", "BT"),
                   {"hist": eng.zeros(4)})
    it, hist, x = solve(ses)
    it2, hist2, x2 = solve(session(A, B, f, g, J1, preS, k=ses.k))
    assert it == it2
    np.testing.assert_array_equal(hist, hist2)
    np.testing.assert_array_equal(x, x2)
    check_against_bpcg_v2(s, f, g, kr.block_jacobi(s.A, blocks), ses.k, it, hist, x)


def test_minres_loop_after_a_pair_plan_of_its_B(hip_engine):
    """A MinresLoop over (A, B) sizes its partials; a Bpcg2Loop on the same B pair-plans it (shorter row blocks);
    the MINRES state is then stale: the library refuses it, and re-sizing makes it consistent again.  A MINRES solve
    afterwards meets the oracle."""
    import hipla
    from hipla import fused
    from minres import MinRes
    eng = hip_engine
    require_guard(eng)
    seen = []
    for dim, n, inflate in CANDIDATES:
        s, f, g, A, B = system(dim, n, inflate)
        preA, preS = hipla.JacobiPreconditioner(A), hipla.DiagonalMatrix(1.0 / s.mass)
        K = hipla.BlockMatrix([[A, B.CreateTranspose()], [B, None]])
        Cm = hipla.BlockMatrix([[preA, None], [None, preS]])
        vec = lambda: hipla.BlockVector([hipla.Vector(s.n_u), hipla.Vector(s.n_p)])
        loop = fused.MinresLoop.try_create(K, Cm, vec(), [vec() for _ in range(3)], [vec() for _ in range(3)],
                                           [vec() for _ in range(2)], vec())
        assert loop is not None
        st = loop.state
        assert workspace(eng.lib.nss_minres_workspace, st, 3) == caps(st, 3)
        nblk = B.handle.info()["row_blocks"]
        session(A, B, f, g, preA, preS)                           # Bpcg2Loop.__init__: B.handle.plan_for_pairs()
        seen.append((dim, n, inflate, nblk, B.handle.info()["row_blocks"]))
        if B.handle.info()["row_blocks"] != nblk:
            break
    else:
        pytest.fail("no system size where the pair-plan moves B's row-block count: %r" % (seen,))
    assert workspace(eng.lib.nss_minres_workspace, st, 3) != caps(st, 3)
    assert_refused(eng, lambda p: eng.lib.nss_minres_iterate(p, 1, 2, eng.stream), st, ("A", "B", "BT"),
                   {"hist": eng.zeros(4)})
    loop.partials = fused.fit_partials(eng, st, eng.lib.nss_minres_workspace, ("A", "B", "BT"), loop.partials)
    assert workspace(eng.lib.nss_minres_workspace, st, 3) == caps(st, 3)
    with contextlib.redirect_stdout(io.StringIO()):
        um, errs = MinRes(mat=K, pre=Cm, rhs=hipla.BlockVector([hipla.Vector.from_numpy(f), hipla.Vector.from_numpy(g)]),
                          maxsteps=2000, tol=1e-9, printrates=False)
    _, _, m_ref, _ = kr.minres(s.A, s.B, kr.jacobi(s.A), kr.diag_inverse(s.mass), f, g, maxsteps=2000, tol=1e-9)
    np.testing.assert_allclose(errs[:40], m_ref[:40], rtol=1e-8)
    b = np.concatenate([f, g])
    assert np.linalg.norm(b - s.saddle_matrix() @ um.numpy()) < 1e-6 * np.linalg.norm(b)


def test_cg_loop_refuses_after_its_matrix_was_replanned(hip_engine):
    """The CG loop (hipla.CGSolver's native loop) over A, A then re-planned around block-Jacobi blocks: refused while
    stale; its next solve re-sizes and matches a loop built afterwards bit for bit, and the oracle's CG."""
    import hipla
    from hipla import fused
    eng = hip_engine
    require_guard(eng)
    s = mac_stokes(2, 24, 0.01)
    A = hipla.SparseMatrix.from_scipy(s.A)
    pre = hipla.JacobiPreconditioner(A)
    loop = fused.CgLoop.try_create(A, pre)
    st = loop.state
    gen = A.handle.plan_generation()
    A.handle.plan_for_blocks(hipla.BlockJacobi(A, s.line_blocks(3)).handle)
    assert A.handle.plan_generation() > gen
    assert_refused(eng, lambda p: eng.lib.nss_cg_iterate(p, 0, 1, eng.stream), st, ("A",),
                   {"hist": eng.zeros(4), "x": eng.zeros(s.n_u)})
    b = np.random.default_rng(3).standard_normal(s.n_u)
    x1, x2 = hipla.Vector(s.n_u), hipla.Vector(s.n_u)
    it1, e1 = loop.solve(hipla.Vector.from_numpy(b).buf, x1.buf, 1e-10, 2000)
    it2, e2 = fused.CgLoop.try_create(A, pre).solve(hipla.Vector.from_numpy(b).buf, x2.buf, 1e-10, 2000)
    assert it1 == it2 and e1 == e2
    np.testing.assert_array_equal(x1.numpy(), x2.numpy())
    x_ref = kr.cg(s.A, b, kr.jacobi(s.A), tol=1e-10, maxsteps=2000)[0]
    assert np.linalg.norm(x1.numpy() - x_ref) < 1e-6 * np.linalg.norm(x_ref)


def test_auxiliary_amg_handle_refuses_a_replanned_level(hip_engine):
    """nss_amg_create_auxiliary re-plans a hierarchy shared by its components (joint cycle) and records the plan
    generations of the level matrices; a later re-plan of a level matrix through a public entry point makes the
    handle refuse instead of launching with stale row-block descriptors, also when the row-block array comes back at
    the same address."""
    import hipla
    eng = hip_engine
    require_guard(eng)
    s = mac_stokes(2, 24, 0.01)
    space = s.auxiliary_space()
    lap = hipla.SparseMatrix.from_scipy(space["laplacians"][0])
    comp = hipla.SmoothedAggregationAMG(lap, coarse_size=50)
    assert len(comp.level_sizes) >= 2
    import scipy.sparse as sp
    n0 = comp.level_sizes[0]
    T = sp.block_diag([sp.identity(n0), sp.identity(n0)]).tocsr()   # two components on one hierarchy
    transform = hipla.SparseMatrix.from_scipy(T)
    gen0 = lap.handle.plan_generation()
    aux = hipla.AuxiliarySpaceAMG(transform, [comp, comp])      # shared hierarchy: joint cycle, re-plans the levels
    assert lap.handle.plan_generation() > gen0
    x = hipla.Vector.from_numpy(np.random.default_rng(4).standard_normal(2 * n0))
    y0 = hipla.Vector(2 * n0)
    aux.Mult(x, y0)
    gen = lap.handle.plan_generation()
    pairs = [list(range(i, min(i + 2, n0))) for i in range(0, n0, 2)]          # runs of consecutive dofs tiling the rows
    planned = lap.handle.plan_for_blocks(hipla.BlockJacobi(lap, pairs).handle)
    assert lap.handle.plan_generation() > gen, planned
    y = hipla.Vector(2 * n0)
    with pytest.raises(Exception, match="re-planned"):
        aux.Mult(x, y)
    # a handle created now describes the new plan and cycles as before (per-row sums keep their bits)
    aux2 = hipla.AuxiliarySpaceAMG(transform, [comp, comp])
    aux2.Mult(x, y)
    np.testing.assert_allclose(y.numpy(), y0.numpy(), rtol=1e-13, atol=1e-13 * np.abs(y0.numpy()).max())
