"""Solver-level parity on the GPU: the three drop-in entry points (HIP engine, through the
C ABI) against (a) the golden vectors produced by the reference's unmodified files and
(b) the CPU oracle on the same assembled matrices.

Tolerance contract: residual history within 1e-8 relative over the
fixture's stable window W; iterations within conftest.iteration_tolerance; solution / true residual to
1e-8 (relative to |x| resp. |b|, scaled by the tolerance the run was stopped at)."""

import contextlib
import glob
import io
import os
import re

import numpy as np
import pytest

from conftest import GOLDEN, golden_path, iteration_tolerance
from golden_cases import Case
from oracle import krylov_ref as kr
from staggered_grid import diffusion_2d, mac_stokes

pytestmark = pytest.mark.gpu

CASES = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(GOLDEN, "stokes*.npz")))


class Form:
    def __init__(self, mat):
        self.mat, self.condense = mat, False


class CondensedFormOf:
    """`blfA` with `condense = True` over the operators of a golden case
    (solvers/bramblepasciak_new.py:11-17,88,105-109)."""

    def __init__(self, parts):
        import hipla
        self.condense = True
        self.mat = hipla.SparseMatrix.from_scipy(parts["mat"])
        for key in ("inner_matrix", "inner_solve", "harmonic_extension", "harmonic_extension_trans"):
            setattr(self, key, hipla.SparseMatrix.from_scipy(parts[key]))


def case_operands(d):
    """Device operands of a golden fixture: (Case, blfA, A, B, preA, preS)."""
    import hipla
    c = Case(d)
    s = c.system
    A = hipla.SparseMatrix.from_scipy(s.A)
    B = hipla.SparseMatrix.from_scipy(s.B)
    blfA = CondensedFormOf(c.parts) if c.condense else Form(A)
    if c.blocks is None:
        preA = hipla.DiagonalMatrix(c.jacobi_diagonal()) if c.condense else hipla.JacobiPreconditioner(A)
    else:
        preA = hipla.BlockJacobi(blfA.mat, c.blocks)
    return c, blfA, A, B, preA, hipla.DiagonalMatrix(1.0 / s.mass)


def operands(d):
    c, _, A, B, preA, preS = case_operands(d)
    assert not c.condense
    return c.system, c.f, c.g, A, B, preA, preS


@contextlib.contextmanager
def fused_loops_counted():
    """Counts the runs of the device-resident loops, so that a test can assert that the fused HIP
    path (not the statement-by-statement protocol path) produced what it compares."""
    from hipla import fused
    counts = {"bpcg2": 0, "bpcg1": 0, "minres": 0}
    saved = {}
    for key, cls in (("bpcg2", fused.Bpcg2Loop), ("bpcg1", fused.Bpcg1Loop), ("minres", fused.MinresLoop)):
        saved[cls] = cls.run

        def counting(self, *a, _key=key, _orig=cls.run, **kw):
            counts[_key] += 1
            return _orig(self, *a, **kw)
        cls.run = counting
    try:
        yield counts
    finally:
        for cls, orig in saved.items():
            cls.run = orig


def check_history(h, ref, window, rtol=1e-8):
    w = min(int(window), len(h), len(ref))
    rel = np.abs(np.asarray(h[:w]) - ref[:w]) / np.abs(ref[:w])
    assert rel.max() <= rtol, rel.max()


def check_iterations(it, ref, d):
    tol = iteration_tolerance(d)
    assert abs(int(it) - int(ref)) <= tol, (it, ref, tol)


def check_solution(x, s, f, g, d):
    b = np.concatenate([f, g])
    res = np.linalg.norm(b - s.saddle_matrix() @ x)
    assert res <= 10 * max(float(d["residual"]), 1e-12 * float(d["b_norm"]))
    assert abs(np.linalg.norm(x) - float(d["x_norm"])) <= 1e-6 * float(d["x_norm"])
    np.testing.assert_allclose(x[d["sample_idx"]], d["sample_val"], rtol=0, atol=1e-6 * np.abs(x).max())


@pytest.mark.parametrize("case", CASES)
def test_entry_points_match_goldens(hip_engine, case):
    import hipla
    from bramble_pasciak_cg import bramble_pasciak_cg
    from minres import MinRes
    from solvers.bramblepasciak_new import BramblePasciakCG
    d = np.load(golden_path(case))
    c, blfA, A, B, preA, preS = case_operands(d)
    s, f, g = c.system, c.f, c.g
    fv, gv = hipla.Vector.from_numpy(f), hipla.Vector.from_numpy(g)
    solver = str(d["solver"])
    out = io.StringIO()
    with fused_loops_counted() as counts:
        x = _run_entry_point(d, solver, c, blfA, A, B, preA, preS, fv, gv, out)
    assert counts[solver] == 1, "the fused device loop did not run: %r" % (counts,)
    check_solution(x, s, f, g, d)


def _run_entry_point(d, solver, c, blfA, A, B, preA, preS, fv, gv, out):
    import hipla
    from bramble_pasciak_cg import bramble_pasciak_cg
    from minres import MinRes
    from solvers.bramblepasciak_new import BramblePasciakCG
    s = c.system
    if solver == "bpcg1":
        with contextlib.redirect_stdout(out):
            sol, errors = bramble_pasciak_cg(A, B, None, preA, preS, fv, gv, tolerance=float(d["tol"]),
                                             max_steps=int(d["maxsteps"]), print_rates=False)
        k = float(re.search(r"scale factor:\s+(\S+)", out.getvalue()).group(1))
        assert abs(k - float(d["k"])) <= 1e-8 * k
        check_history(errors, d["errors"], d["window"])
        check_iterations(len(errors) - 1, d["iterations"], d)
        x = sol.numpy()
    elif solver == "bpcg2":
        sol = hipla.BlockVector([hipla.Vector(s.n_u), hipla.Vector(s.n_p)])
        with contextlib.redirect_stdout(out):
            it, seconds = BramblePasciakCG(blfA, Form(B), None, fv, gv, preA, preS, sol, tol=float(d["tol"]),
                                           maxsteps=int(d["maxsteps"]), printrates=True)
        text = out.getvalue()
        hist = np.array([float(m) for m in re.findall(r"it =\s+\d+\s+err =\s+(\S+)", text)])
        err0 = float(re.search(r"err0 (\S+)", text).group(1))
        assert abs(err0 - float(d["err0"])) <= 1e-8 * err0
        assert len(hist) == it + 1 and seconds > 0
        check_history(hist, d["history"], d["window"])
        check_iterations(it, d["iterations"], d)
        x = sol.numpy()
    else:
        K = hipla.BlockMatrix([[A, B.T], [B, None]])
        Cm = hipla.BlockMatrix([[preA, None], [None, preS]])
        with contextlib.redirect_stdout(out):
            u, errors = MinRes(mat=K, pre=Cm, rhs=hipla.BlockVector([fv, gv]), maxsteps=int(d["maxsteps"]),
                               tol=float(d["tol"]), printrates=False)
        check_history(errors, d["errors"], d["window"])
        check_iterations(len(errors) - 1, d["iterations"], d)
        assert ("Warning" in out.getvalue()) == bool(d["warned"])
        x = u.numpy()
    return x


def test_protocol_path_with_user_subclasses(hip_engine):
    """User BaseMatrix subclasses (here: operators hiding the native types) force the
    protocol path; it must agree with the native/fused path and the goldens."""
    import hipla
    from bramble_pasciak_cg import bramble_pasciak_cg
    from minres import MinRes
    from solvers.bramblepasciak_new import BramblePasciakCG

    class Opaque(hipla.BaseMatrix):
        def __init__(self, inner):
            super().__init__()
            self.inner = inner

        def Mult(self, x, y):
            y.data = self.inner * x

        def MultTrans(self, x, y):
            y.data = self.inner.T * x

        def Height(self):
            return self.inner.height

        def Width(self):
            return self.inner.width

        def CreateTranspose(self):
            return Opaque(self.inner.T)

    d = np.load(golden_path("stokes2d_n12_jacobi_bpcg2"))
    s, f, g, A, B, preA, preS = operands(d)
    fv, gv = hipla.Vector.from_numpy(f), hipla.Vector.from_numpy(g)
    sol = hipla.BlockVector([hipla.Vector(s.n_u), hipla.Vector(s.n_p)])
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        it, _ = BramblePasciakCG(Form(A), Form(B), None, fv, gv, Opaque(preA), Opaque(preS), sol,
                                 tol=float(d["tol"]), maxsteps=int(d["maxsteps"]))
    hist = np.array([float(m) for m in re.findall(r"it =\s+\d+\s+err =\s+(\S+)", out.getvalue())])
    check_history(hist, d["history"], d["window"])
    check_iterations(it, d["iterations"], d)
    check_solution(sol.numpy(), s, f, g, d)

    d = np.load(golden_path("stokes2d_n12_jacobi_bpcg1"))
    with contextlib.redirect_stdout(io.StringIO()):
        x, errors = bramble_pasciak_cg(A, B, None, Opaque(preA), preS, fv, gv, tolerance=float(d["tol"]),
                                       max_steps=int(d["maxsteps"]), print_rates=False)
    check_history(errors, d["errors"], d["window"])
    check_solution(x.numpy(), s, f, g, d)

    d = np.load(golden_path("stokes2d_n12_jacobi_minres"))
    K = hipla.BlockMatrix([[Opaque(A), B.T], [B, None]])
    Cm = hipla.BlockMatrix([[preA, None], [None, Opaque(preS)]])
    with contextlib.redirect_stdout(io.StringIO()):
        u, errors = MinRes(mat=K, pre=Cm, rhs=hipla.BlockVector([fv, gv]), maxsteps=int(d["maxsteps"]),
                           tol=float(d["tol"]), printrates=False)
    check_history(errors, d["errors"], d["window"])
    check_solution(u.numpy(), s, f, g, d)


def test_quirks(hip_engine):
    import hipla
    from bramble_pasciak_cg import bramble_pasciak_cg
    from minres import MinRes
    from solvers.bramblepasciak_new import BramblePasciakCG
    rng = np.random.default_rng(7)
    d = np.load(golden_path("quirk_minres_absolute_guard"))
    s, f, g, A, B, preA, preS = operands(d)
    warm_u, warm_p = 0.1 * rng.standard_normal(s.n_u), 0.1 * rng.standard_normal(s.n_p)
    K = hipla.BlockMatrix([[A, B.T], [B, None]])
    Cm = hipla.BlockMatrix([[preA, None], [None, preS]])

    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        u, errors = MinRes(mat=K, pre=Cm, rhs=hipla.BlockVector([hipla.Vector.from_numpy(1e-3 * f),
                                                                  hipla.Vector.from_numpy(g)]),
                           maxsteps=int(d["maxsteps"]), tol=float(d["tol"]), printrates=False)
    assert "Warning" in out.getvalue() and bool(d["warned"])       # absolute guard exit warns
    check_iterations(len(errors) - 1, d["iterations"], d)

    d = np.load(golden_path("quirk_minres_warm_start"))
    sol = hipla.BlockVector([hipla.Vector.from_numpy(warm_u), hipla.Vector.from_numpy(warm_p)])
    with contextlib.redirect_stdout(io.StringIO()):
        u, errors = MinRes(mat=K, pre=Cm, rhs=hipla.BlockVector([hipla.Vector.from_numpy(f), hipla.Vector.from_numpy(g)]),
                           sol=sol, initialize=False, maxsteps=int(d["maxsteps"]), tol=float(d["tol"]), printrates=False)
    assert u is sol                                                 # caller storage updated in place
    check_iterations(len(errors) - 1, d["iterations"], d)
    np.testing.assert_allclose(errors[:60], d["errors"][:60], rtol=1e-8)
    assert abs(np.linalg.norm(u.numpy()) - float(d["x_norm"])) < 1e-6 * float(d["x_norm"])

    d = np.load(golden_path("quirk_bpcg2_zero_rhs"))
    sol = hipla.BlockVector([hipla.Vector(s.n_u), hipla.Vector(s.n_p)])
    with contextlib.redirect_stdout(io.StringIO()):
        ret = BramblePasciakCG(Form(A), Form(B), None, hipla.Vector(s.n_u), hipla.Vector(s.n_p), preA, preS, sol)
    assert ret is sol and bool(d["returned_solution_object"])       # bare vector, not a tuple

    for name in ("quirk_bpcg2_warm_start", "quirk_bpcg2_abs_err"):
        d = np.load(golden_path(name))
        sol = hipla.BlockVector([hipla.Vector.from_numpy(warm_u), hipla.Vector.from_numpy(warm_p)])
        out = io.StringIO()
        with contextlib.redirect_stdout(out):
            it, _ = BramblePasciakCG(Form(A), Form(B), None, hipla.Vector.from_numpy(f), hipla.Vector.from_numpy(g),
                                     preA, preS, sol, tol=float(d["tol"]), maxsteps=int(d["maxsteps"]),
                                     initialize=bool(d["initialize"]), rel_err=bool(d["rel_err"]))
        hist = np.array([float(m) for m in re.findall(r"it =\s+\d+\s+err =\s+(\S+)", out.getvalue())])
        check_iterations(it, d["iterations"], d)
        np.testing.assert_allclose(hist[:40], d["history"][:40], rtol=1e-8)
        assert abs(np.linalg.norm(sol.numpy()) - float(d["x_norm"])) < 1e-6 * float(d["x_norm"])

    d = np.load(golden_path("quirk_bpcg1_warm_start_maxsteps"))
    sol = hipla.BlockVector([hipla.Vector.from_numpy(warm_u), hipla.Vector.from_numpy(warm_p)])
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        s2, errors = bramble_pasciak_cg(A, B, None, preA, preS, hipla.Vector.from_numpy(f), hipla.Vector.from_numpy(g),
                                        solution=sol, tolerance=float(d["tol"]), max_steps=int(d["maxsteps"]),
                                        print_rates=False)
    assert s2 is sol and "Warning" in out.getvalue()
    assert len(errors) == int(d["iterations"])
    np.testing.assert_allclose(errors, d["errors"], rtol=1e-7)


def test_cfg1_heat_plumbing(hip_engine):
    """cfg1: SpMV + InnerProduct + AXPY on the 64x64 diffusion matrix -- Gram-Schmidt over a
    Krylov basis and the Galerkin projection (orthonormalization.py:5-16, heat.py:109-118)
    and a plain CG written against the protocol."""
    import hipla
    from math import sqrt
    d = np.load(golden_path("cfg1_heat_plumbing"))
    M = diffusion_2d(64)
    Mh = hipla.SparseMatrix.from_scipy(M)
    x0 = np.random.default_rng(int(d["seed"])).standard_normal(M.shape[0])
    basis = [hipla.Vector.from_numpy(x0)]
    for _ in range(4):
        nxt = basis[-1].CreateVector()
        nxt.data = Mh * basis[-1]
        basis.append(nxt)
    for _ in range(3):
        for j in range(5):
            for i in range(j):
                basis[j].data -= hipla.InnerProduct(basis[i], basis[j]) / hipla.InnerProduct(basis[i], basis[i]) * basis[i]
            basis[j].data = 1 / hipla.Norm(basis[j]) * basis[j]
    gal = np.zeros((5, 5))
    res = basis[0].CreateVector()
    for c in range(5):
        res.data = Mh * basis[c]
        for r in range(5):
            gal[r, c] = hipla.InnerProduct(basis[r], res)
    # the monomial Krylov basis is ill-conditioned: compare the well-conditioned invariants
    np.testing.assert_allclose(np.linalg.eigvalsh(gal), np.linalg.eigvalsh(d["galerkin"]), rtol=1e-7)
    gram = np.array([[hipla.InnerProduct(a, b) for b in basis] for a in basis])
    np.testing.assert_allclose(gram, np.eye(5), atol=1e-12)

    b = hipla.Vector.from_numpy(x0)
    x, r, p, q = (b.CreateVector() for _ in range(4))
    x[:] = 0
    r.data = b
    p.data = r
    rz = hipla.InnerProduct(r, r)
    hist = [sqrt(rz)]
    for _ in range(500):
        q.data = Mh * p
        alpha = rz / hipla.InnerProduct(p, q)
        x.data += alpha * p
        r.data -= alpha * q
        rz_new = hipla.InnerProduct(r, r)
        hist.append(sqrt(rz_new))
        if hist[-1] < 1e-10 * hist[0]:
            break
        p.data = r + (rz_new / rz) * p
        rz = rz_new
    assert len(hist) - 1 == int(d["cg_iterations"])
    np.testing.assert_allclose(hist, d["cg_history"], rtol=1e-8)
    assert abs(np.linalg.norm(x.numpy()) - float(d["cg_x_norm"])) < 1e-9 * float(d["cg_x_norm"])


def test_fused_bpcg2_is_selected_and_agrees_with_protocol_path(hip_engine):
    """Native operands must take the device-resident loop (nss_bpcg2_*); forcing the protocol
    path on the same operands has to give the same history inside the stable window."""
    import hipla
    from hipla import fused
    from solvers.bramblepasciak_new import BpcgSession, BramblePasciakCG
    for case in ("stokes3d_n10_bjac_bpcg2", "stokes2d_n24_jacobi_bpcg2"):
        d = np.load(golden_path(case))
        s, f, g, A, B, preA, preS = operands(d)
        results = {}
        for mode in ("fused", "protocol"):
            fused.ENABLED = mode == "fused"
            try:
                sol = hipla.BlockVector([hipla.Vector(s.n_u), hipla.Vector(s.n_p)])
                with contextlib.redirect_stdout(io.StringIO()):
                    ses = BpcgSession(Form(A), Form(B), None, hipla.Vector.from_numpy(f), hipla.Vector.from_numpy(g),
                                      preA, preS, sol=sol)
                assert (ses.fused is not None) == (mode == "fused")
                out = io.StringIO()
                sol = hipla.BlockVector([hipla.Vector(s.n_u), hipla.Vector(s.n_p)])
                with contextlib.redirect_stdout(out):
                    it, _ = BramblePasciakCG(Form(A), Form(B), None, hipla.Vector.from_numpy(f),
                                             hipla.Vector.from_numpy(g), preA, preS, sol, tol=float(d["tol"]),
                                             maxsteps=int(d["maxsteps"]))
                hist = np.array([float(m) for m in re.findall(r"it =\s+\d+\s+err =\s+(\S+)", out.getvalue())])
                results[mode] = (it, hist, sol.numpy())
            finally:
                fused.ENABLED = True
        w = int(d["window"])
        np.testing.assert_allclose(results["fused"][1][:w], results["protocol"][1][:w], rtol=1e-8)
        check_iterations(results["fused"][0], results["protocol"][0], d)
        xf, xp = results["fused"][2], results["protocol"][2]
        assert np.linalg.norm(xf - xp) <= 1e-6 * np.linalg.norm(xp)


def test_fused_bpcg2_frozen_at_break_and_maxsteps_warning(hip_engine):
    """The done flag freezes the state at the reference's `break`: polling late (large chunks) or
    early (chunks of 1) must return the same iteration index and the same solution bits."""
    import hipla
    from solvers.bramblepasciak_new import BpcgSession
    d = np.load(golden_path("stokes3d_n6_jacobi_bpcg2"))
    s, f, g, A, B, preA, preS = operands(d)
    outs = []
    for chunk in (1, 7, 1000):
        sol = hipla.BlockVector([hipla.Vector(s.n_u), hipla.Vector(s.n_p)])
        with contextlib.redirect_stdout(io.StringIO()):
            ses = BpcgSession(Form(A), Form(B), None, hipla.Vector.from_numpy(f), hipla.Vector.from_numpy(g),
                              preA, preS, sol=sol)
        ses.first_direction()
        it, hist, conv = ses.fused.run(ses.wdn, ses.err0, 1e-8, True, 2000, poll_every=chunk)
        assert conv
        outs.append((it, hist.copy(), sol.numpy()))
    for it, hist, x in outs[1:]:
        assert it == outs[0][0]
        np.testing.assert_array_equal(hist, outs[0][1])
        np.testing.assert_array_equal(x, outs[0][2])
    # not converging within maxsteps: it = maxsteps-1 and the warning is printed
    from solvers.bramblepasciak_new import BramblePasciakCG
    sol = hipla.BlockVector([hipla.Vector(s.n_u), hipla.Vector(s.n_p)])
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        it, _ = BramblePasciakCG(Form(A), Form(B), None, hipla.Vector.from_numpy(f), hipla.Vector.from_numpy(g),
                                 preA, preS, sol, tol=1e-30, maxsteps=9)
    assert it == 8 and "Warning: BPCG did not converge" in out.getvalue()


@pytest.mark.parametrize("name", ["stokes3d_n10_bjac", "stokes2d_n24_jacobi"])
def test_streaming_loads_do_not_change_a_bit(hip_engine, name):
    """The element-wise kernels of the three fused loops load the vector operands they do not read again with
    streaming (non-temporal) loads from 20 MB per vector on -- a cache policy, chosen per launch
    (nss_stream_loads_mode: automatic / never / always).  Forced on and off here (with the row-per-lane kernel for
    B^T, which carries the streaming variant of C1): identical histories and solutions."""
    import hipla
    from bramble_pasciak_cg import bramble_pasciak_cg
    from minres import MinRes
    from solvers.bramblepasciak_new import BramblePasciakCG
    results = {}
    for mode in (0, 1):
        with hip_engine.overrides(direct_rows=0, stream_loads=mode):
            for solver in ("bpcg2", "bpcg1", "minres"):
                d = np.load(golden_path("%s_%s" % (name, solver)))
                c, blfA, A, B, preA, preS = case_operands(d)
                s = c.system
                fv, gv = hipla.Vector.from_numpy(c.f), hipla.Vector.from_numpy(c.g)
                out = io.StringIO()
                with fused_loops_counted() as counts, contextlib.redirect_stdout(out):
                    if solver == "bpcg2":
                        sol = hipla.BlockVector([hipla.Vector(s.n_u), hipla.Vector(s.n_p)])
                        BramblePasciakCG(blfA, Form(B), None, fv, gv, preA, preS, sol, tol=float(d["tol"]),
                                         maxsteps=int(d["maxsteps"]), printrates=True)
                        hist = np.array([float(m) for m in re.findall(r"it =\s+\d+\s+err =\s+(\S+)", out.getvalue())])
                        x = sol.numpy()
                    elif solver == "bpcg1":
                        sol, errors = bramble_pasciak_cg(A, B, None, preA, preS, fv, gv, tolerance=float(d["tol"]),
                                                         max_steps=int(d["maxsteps"]), print_rates=False)
                        hist, x = np.array(errors), sol.numpy()
                    else:
                        K = hipla.BlockMatrix([[A, B.T], [B, None]])
                        Cm = hipla.BlockMatrix([[preA, None], [None, preS]])
                        u, errors = MinRes(mat=K, pre=Cm, rhs=hipla.BlockVector([fv, gv]), maxsteps=int(d["maxsteps"]),
                                           tol=float(d["tol"]), printrates=False)
                        hist, x = np.array(errors), u.numpy()
                assert counts[solver] == 1
                check = d["history"] if solver == "bpcg2" else d["errors"]
                check_history(hist, check, d["window"])
                results[mode, solver] = (hist, x)
    for solver in ("bpcg2", "bpcg1", "minres"):
        np.testing.assert_array_equal(results[1, solver][0], results[0, solver][0])
        np.testing.assert_array_equal(results[1, solver][1], results[0, solver][1])


@pytest.mark.parametrize("name", ["stokes3d_n10_bjac", "stokes2d_n24_jacobi"])
def test_row_per_lane_kernel_in_the_fused_loops(hip_engine, name):
    """B^T (two entries per row) multiplied by the row-per-lane kernel from its fixed-width copy instead of by the
    stream kernel (csr_direct_kernel; automatic from 2^21 rows on, forced here): the three fused loops produce the
    same histories and solutions bit for bit -- the row sums are formed in the same order without fused
    multiply-adds, and no dot product is grouped by B^T's row blocks."""
    import hipla
    from bramble_pasciak_cg import bramble_pasciak_cg
    from minres import MinRes
    from solvers.bramblepasciak_new import BramblePasciakCG
    results = {}
    for mode, rows in (("stream", -1), ("rows", 0)):
        with hip_engine.overrides(direct_rows=rows):
            for solver in ("bpcg2", "bpcg1", "minres"):
                d = np.load(golden_path("%s_%s" % (name, solver)))
                c, blfA, A, B, preA, preS = case_operands(d)
                s = c.system
                assert (B.T.handle.info()["operand_form"] == "rows") == (mode == "rows")
                fv, gv = hipla.Vector.from_numpy(c.f), hipla.Vector.from_numpy(c.g)
                out = io.StringIO()
                with fused_loops_counted() as counts, contextlib.redirect_stdout(out):
                    if solver == "bpcg2":
                        sol = hipla.BlockVector([hipla.Vector(s.n_u), hipla.Vector(s.n_p)])
                        BramblePasciakCG(blfA, Form(B), None, fv, gv, preA, preS, sol, tol=float(d["tol"]),
                                         maxsteps=int(d["maxsteps"]), printrates=True)
                        hist = np.array([float(m) for m in re.findall(r"it =\s+\d+\s+err =\s+(\S+)", out.getvalue())])
                        x = sol.numpy()
                    elif solver == "bpcg1":
                        sol, errors = bramble_pasciak_cg(A, B, None, preA, preS, fv, gv, tolerance=float(d["tol"]),
                                                         max_steps=int(d["maxsteps"]), print_rates=False)
                        hist, x = np.array(errors), sol.numpy()
                    else:
                        K = hipla.BlockMatrix([[A, B.T], [B, None]])
                        Cm = hipla.BlockMatrix([[preA, None], [None, preS]])
                        u, errors = MinRes(mat=K, pre=Cm, rhs=hipla.BlockVector([fv, gv]), maxsteps=int(d["maxsteps"]),
                                           tol=float(d["tol"]), printrates=False)
                        hist, x = np.array(errors), u.numpy()
                assert counts[solver] == 1
                results[mode, solver] = (hist, x)
    for solver in ("bpcg2", "bpcg1", "minres"):
        np.testing.assert_array_equal(results["rows", solver][0], results["stream", solver][0])
        np.testing.assert_array_equal(results["rows", solver][1], results["stream", solver][1])


@pytest.mark.parametrize("case", ["stokes3d_n10_bjac_bpcg2", "stokes2d_n24_jacobi_bpcg2",
                                  "stokes3d_n5_facet_x12_bpcg2", "stokes2d_n16_facet_x5_bpcg2",
                                  "stokes3d_n8_bjac_cond_bpcg2"])
def test_compact_plan_equals_eight_phase_form_bit_for_bit(hip_engine, case):
    """The single-GPU loop issues three dependent launches per iteration (C1, C23, C4: books of the
    previous iteration and the dot-product sums folded into the consuming kernels, A and B rows in
    one launch, operands beta*s1 + w1 and t1 - s0 formed on the fly) where the eight-phase form -- which
    the row-partitioned loop keeps -- issues eight.  Same floating-point operations per lane and
    the same summation tree: identical bits, with the sums folded or in their stand-alone kernels,
    including the iteration at which the stop test fires."""
    import hipla
    from solvers.bramblepasciak_new import BpcgSession
    d = np.load(golden_path(case))
    c, blfA, A, B, preA, preS = case_operands(d)
    s = c.system

    def run(form, nit, tol):
        sol = hipla.BlockVector([hipla.Vector(s.n_u), hipla.Vector(s.n_p)])
        with contextlib.redirect_stdout(io.StringIO()):
            ses = BpcgSession(blfA, Form(B), None, hipla.Vector.from_numpy(c.f), hipla.Vector.from_numpy(c.g),
                              preA, preS, sol=sol)
        loop = ses.fused
        assert loop is not None
        ses.first_direction()
        loop.start(ses.wdn, ses.err0, tol, True, nit)
        it = 0
        while it < nit:                            # uneven chunks: the books of a chunk's last iteration
            end = min(nit, it + 1 + (it % 5))      # are done by the poll, the others by the next C1
            (loop.enqueue_classic if form == "classic" else loop.enqueue)(it, end)
            it = end
            done, it_final, last = loop.poll()
            if done:
                break
        final = it_final if done else nit - 1
        return done, final, loop.history(final).copy(), sol.numpy(), hip_engine.to_host(loop.scal).copy()

    free = run("classic", 40, 0.0)
    k_stop = int(np.argmin(free[2][:30]))              # the stop test fires first at this iteration ...
    tol_stop = free[2][k_stop] * (1.0 + 1e-12) / float(d["err0"]) if k_stop > 0 else 0.0
    for tol in (tol_stop, 0.0):
        ref = run("classic", 40, tol)
        if tol > 0.0:
            assert ref[0] and 0 < ref[1] <= k_stop + 1, (ref[:2], k_stop)   # ... (tested one iteration late, :243-247)
        assert np.all(np.isfinite(ref[2])) and len(ref[2]) == ref[1] + 1
        for mode in (1, 0, -1):
            with hip_engine.overrides(bpcg2_fold=mode):
                got = run("compact", 40, tol)
            assert got[0] == ref[0] and got[1] == ref[1], (mode, tol, got[:2], ref[:2])
            np.testing.assert_array_equal(got[2], ref[2])           # history
            np.testing.assert_array_equal(got[3], ref[3])           # solution
            np.testing.assert_array_equal(got[4][:5], ref[4][:5])   # wd, as_s, wdn, alpha, beta
    w = min(int(d["window"]), 40)
    np.testing.assert_allclose(ref[2][:w], d["history"][:w], rtol=1e-8)


@pytest.mark.parametrize("dim,n,inflate,bs", [(3, 20, 1, 3), (2, 90, 1, 3), (2, 40, 1, 2), (2, 24, 4, 1), (3, 56, 1, 3)])
def test_block_jacobi_applied_in_the_epilogue_of_c1(hip_engine, dim, n, inflate, bs):
    """Block Jacobi alone as preA (templates/NavierStokesSIMPLE_iterative.py:360-373,383): with B^T's row blocks
    planned around the Jacobi blocks (nss_csr_plan_for_blocks) C1 applies t1 = k J t0 itself -- the row block's t0
    passes through LDS, one lane per Jacobi block -- instead of a launch that reads t0 back.  (i) the re-planned B^T
    multiplies to the bits of the original plan; (ii) history and solution equal the stand-alone apply's bit for bit,
    for the row-per-lane kernel (3-D, large 2-D), the stream kernel (small / wide B^T) and ragged line ends;
    (iii) blocks that do not tile the rows are declined and the loop runs as before."""
    import hipla
    from solvers.bramblepasciak_new import BpcgSession
    s = mac_stokes(dim, n, 0.01)
    if inflate > 1:
        s = s.inflate(inflate)
    f, g = s.rhs(0)
    xp = hipla.Vector.from_numpy(np.random.default_rng(2).standard_normal(s.n_p))
    BT0 = hipla.SparseMatrix.from_scipy(s.B.T.tocsr())
    y0 = hipla.Vector(s.n_u)
    y0.data = BT0 * xp

    def run(fuse, blocks, nit=30):
        with hip_engine.overrides(fuse_bjac=1 if fuse else 0):                      # (-1, the default: by size)
            A, B = hipla.SparseMatrix.from_scipy(s.A), hipla.SparseMatrix.from_scipy(s.B)
            preA = hipla.BlockJacobi(A, blocks)
            sol = hipla.BlockVector([hipla.Vector(s.n_u), hipla.Vector(s.n_p)])
            with contextlib.redirect_stdout(io.StringIO()):
                ses = BpcgSession(Form(A), Form(B), None, hipla.Vector.from_numpy(f), hipla.Vector.from_numpy(g), preA,
                                  hipla.DiagonalMatrix(1.0 / s.mass), sol=sol)
            loop = ses.fused
            ses.first_direction()
            loop.start(ses.wdn, ses.err0, 0.0, True, nit)
            loop.enqueue(0, nit)
            loop.poll()
            y = hipla.Vector(s.n_u)
            y.data = ses.matBT * xp
            assert loop.c1_applies_preA() == (bool(fuse) and loop.c1_applies_bjac)
            return loop.history(nit - 1).copy(), sol.numpy(), y.numpy(), loop.c1_applies_bjac

    blocks = s.line_blocks(bs)
    apart = run(False, blocks)
    fused = run(True, blocks)
    assert fused[3] and not apart[3]                     # (mode 0: B^T is not even re-planned)
    np.testing.assert_array_equal(fused[2], y0.numpy())                  # (i)
    np.testing.assert_array_equal(fused[0], apart[0])                    # (ii)
    np.testing.assert_array_equal(fused[1], apart[1])
    assert np.all(np.isfinite(fused[0])) and fused[0][-1] < fused[0][0]
    if dim == 2 and n == 40:
        rev = np.ascontiguousarray(np.asarray(blocks)[:, ::-1])          # any block numbering: taken in row order
        a, b = run(False, rev), run(True, rev)
        assert b[3] and not a[3]
        np.testing.assert_array_equal(a[0], b[0])
        np.testing.assert_array_equal(a[1], b[1])
        fewer = np.ascontiguousarray(np.asarray(blocks)[:, :-1])         # (iii) a dof in no block: declined
        declined = run(True, fewer)
        assert not declined[3] and np.all(np.isfinite(declined[0]))


@pytest.mark.parametrize("dim,n,inflate", [(3, 16, 1), (2, 40, 1), (3, 6, 12)])
def test_pair_staged_operands_give_identical_bits(hip_engine, dim, n, inflate):
    """Kernels whose SpMV operand is an expression of two stored vectors -- the rows of B multiply t1 - s0, the rows
    of B^T beta s1 + w1 (solvers/bramblepasciak_new.py:212-213, :206 + :240-241) -- read both vectors from LDS copies
    filled by LDS-DMA when the operand runs of every row block fit twice into the LDS buffer
    (nss_csr_plan_for_pairs re-plans B with 1024-product row blocks to get there).  Same products in the same
    order: (i) the re-planned matrix multiplies to the same bits as before, (ii) the fused loop with the pair-staged
    form gives the bits of the same loop gathering through the window form of the same matrices."""
    import hipla
    from solvers.bramblepasciak_new import BpcgSession
    s = mac_stokes(dim, n, 0.01)
    if inflate > 1:
        s = s.inflate(inflate)
    f, g = s.rhs(0)
    x = hipla.Vector.from_numpy(np.random.default_rng(1).standard_normal(s.n_u))
    B0 = hipla.SparseMatrix.from_scipy(s.B)
    y0 = hipla.Vector(s.n_p)
    y0.data = B0 * x
    blocks_before = B0.handle.info()["row_blocks"]

    def run(nit=30):
        A, B = hipla.SparseMatrix.from_scipy(s.A), hipla.SparseMatrix.from_scipy(s.B)
        preA = hipla.BlockJacobi(A, s.line_blocks(3 if inflate == 1 else 1))
        sol = hipla.BlockVector([hipla.Vector(s.n_u), hipla.Vector(s.n_p)])
        with contextlib.redirect_stdout(io.StringIO()):
            ses = BpcgSession(Form(A), Form(B), None, hipla.Vector.from_numpy(f), hipla.Vector.from_numpy(g), preA,
                              hipla.DiagonalMatrix(1.0 / s.mass), sol=sol)
        loop = ses.fused
        ses.first_direction()
        loop.start(ses.wdn, ses.err0, 0.0, True, nit)
        loop.enqueue(0, nit)
        loop.poll()
        y = hipla.Vector(s.n_p)
        y.data = B * x                                  # the re-planned B, plain SpMV
        return loop.history(nit - 1).copy(), sol.numpy(), B.handle.info(), ses.matBT.handle.info(), y.numpy(), loop

    with hip_engine.overrides(pair_stage=0):
        gathered = run()
    with hip_engine.overrides(pair_stage=-1):
        paired = run()
    np.testing.assert_array_equal(paired[4], y0.numpy())                 # (i)
    np.testing.assert_array_equal(gathered[4], y0.numpy())
    np.testing.assert_array_equal(paired[0], gathered[0])                # (ii) history
    np.testing.assert_array_equal(paired[1], gathered[1])                #      solution
    assert np.all(np.isfinite(paired[0]))
    b_info, bt_info = paired[2], paired[3]
    if inflate == 1:                                                      # grid operators: B re-planned and pair-staged
        assert b_info["operand_form"] == "staged" and b_info["pair_staged"] and paired[5].pair_staged_b
        assert b_info["row_blocks"] >= blocks_before          # (small systems already have short row blocks)
        assert bt_info["pair_staged"] or bt_info["operand_form"] == "rows"


def test_device_resident_lanczos_matches_the_protocol_recurrence(hip_engine):
    """`EigenValues_Preconditioner` (scale factor k: bramble_pasciak_cg.py:68-74, solvers/bramblepasciak_new.py:111-122)
    on native operands runs the Lanczos recurrence resident on the device (csrc/lanczos.hip: un-normalised vectors, the
    dots in the epilogues of the SpMV / block-Jacobi kernels, scalars advanced by the sum kernels; the host reads the
    tridiagonal once per 5 steps).  Same recurrence, same start vector as the statement-by-statement protocol form
    (two host-synchronising dots per step) and as the oracle: Ritz values to 1e-12 / 1e-10, same number of steps --
    for point / block Jacobi, the symmetric Gauss-Seidel sweep, a V-cycle and both forms of MypreA."""
    import hipla
    from hipla import eigen
    from templates.NavierStokesSIMPLE_iterative import MypreA, auxiliary_space_preconditioner
    s = mac_stokes(3, 12, 0.01)
    A = hipla.SparseMatrix.from_scipy(s.A)
    blocks = s.line_blocks(3)
    _, _, aux = auxiliary_space_preconditioner(s)
    G = hipla.BlockGaussSeidel(A, blocks)
    pres = {"jacobi": hipla.JacobiPreconditioner(A), "bjac": hipla.BlockJacobi(A, blocks), "bgs": G,
            "amg": hipla.SmoothedAggregationAMG(A, coarse_size=300), "scaled_bjac": 2.5 * hipla.BlockJacobi(A, blocks),
            "mypre_additive": MypreA(None, Form(A), blocks, GS=False, aux=aux),
            "mypre_multiplicative": MypreA(None, Form(A), blocks, GS=True, aux=aux)}
    calls = []
    orig = eigen._native_lanczos

    def spy(*a, **k):
        out = orig(*a, **k)
        calls.append(out is not None)
        return out

    eigen._native_lanczos = spy
    try:
        for name, pre in pres.items():
            for tol in (1e-3, 1e-10):
                del calls[:]
                native = eigen.EigenValues_Preconditioner(mat=A, pre=pre, tol=tol)
                assert calls == [True], name
                eigen.NATIVE = False
                try:
                    del calls[:]
                    proto = eigen.EigenValues_Preconditioner(mat=A, pre=pre, tol=tol)
                    assert calls == [False]
                finally:
                    eigen.NATIVE = True
                if tol == 1e-3:      # the solvers' setting: a few dozen steps, every Ritz value of the two runs agrees
                    assert len(native) == len(proto), (name, tol, len(native), len(proto))
                    np.testing.assert_allclose(native, proto, rtol=1e-10, atol=1e-12 * abs(proto).max())
                else:                # hundreds of steps without re-orthogonalisation: copies of converged Ritz values
                    # appear at rounding-dependent steps; the extreme values -- what callers use -- still agree
                    assert abs(len(native) - len(proto)) <= 10, (name, len(native), len(proto))
                    assert abs(native.max() - proto.max()) <= 1e-9 * proto.max()
                assert abs(native.min() - proto.min()) <= 1e-12 * proto.max() + 1e-9 * proto.min()
        # ... and the oracle's recurrence on the host
        ref = kr.lanczos_ritz(s.A, kr.block_jacobi(s.A, blocks), tol=1e-3)
        got = eigen.EigenValues_Preconditioner(mat=A, pre=pres["bjac"], tol=1e-3)
        assert len(got) == len(ref) and abs(got.min() - ref.min()) <= 1e-9 * ref.min()
        # an operator that annihilates the start vector: gamma_0 == 0 -> no Ritz values (as the protocol form)
        Z = hipla.DiagonalMatrix(np.zeros(s.n_u))
        assert len(eigen.EigenValues_Preconditioner(mat=A, pre=Z, tol=1e-3)) == 0
    finally:
        eigen._native_lanczos = orig


def test_two_launch_lanczos_step_for_small_systems(hip_engine):
    """Small systems run a Lanczos step in two launches (csrc/lanczos.hip: the rows of A, then one kernel that sums
    both sets of dot partials in every workgroup, keeps the books and applies update + block Jacobi + dot; include/
    nss_krylov.h::nss_lanczos_fold_mode).  Against the five-launch form: the same steps, Ritz values to 1e-10 (the sums
    use another tree), for the all-folded form (A's partials <= 1024), the mixed form (A's sum stand-alone: n = 48) and
    with a breakdown at step 0 (preA A = I) -- in batches whose ends fall on every residue of the step count."""
    import scipy.sparse as sp
    import hipla
    from hipla import eigen

    def ritz(A, pre, mode, tol=1e-3, check_every=5):
        with hip_engine.overrides(lanczos_fold=mode):
            start = A.CreateColVector()
            start.set_from(eigen.lanczos_start_values(0, len(start)))
            out = eigen._native_lanczos(A, pre, start, tol, 400, check_every)
            assert out is not None
            return out

    for n in (10, 48):
        s = mac_stokes(3, n, 0.01)
        A = hipla.SparseMatrix.from_scipy(s.A)
        assert (A.handle.info()["row_blocks"] > 1024) == (n == 48)
        for pre in (hipla.BlockJacobi(A, s.line_blocks(3)), 0.5 * hipla.BlockJacobi(A, s.line_blocks(2))):
            five = ritz(A, pre, 0)
            for mode in (-1, 1):
                two = ritz(A, pre, mode)
                assert len(two) == len(five), (n, mode, len(two), len(five))
                np.testing.assert_allclose(two, five, rtol=1e-10, atol=1e-12 * five.max())
            if n == 10:
                for every in (1, 3, 7):         # other batch ends: the books kernel and the next batch's first kernel
                    a, b = ritz(A, pre, 0, check_every=every), ritz(A, pre, 1, check_every=every)
                    assert len(a) == len(b)
                    np.testing.assert_allclose(b, a, rtol=1e-10, atol=1e-12 * a.max())
    # the start vector is formed on the device: the bits of the numpy form, at any offset (64-bit wrap-around)
    for off in (0, 7, 3_000_000_000, 2 ** 40 + 5):
        buf = hip_engine.zeros(1003)
        hip_engine.lanczos_start_values(buf, off)
        assert np.array_equal(hip_engine.to_host(buf), eigen.lanczos_start_values(off, 1003)), off
    # breakdown: block-diagonal A with the blocks of the preconditioner -> preA A = I, gamma_1 = 0 at step 0
    rng = np.random.default_rng(5)
    blocks, mats = [], []
    for b in range(700):
        m = rng.standard_normal((3, 3))
        mats.append(m @ m.T + 3.0 * np.eye(3))
        blocks.append([3 * b, 3 * b + 1, 3 * b + 2])
    A = hipla.SparseMatrix.from_scipy(sp.block_diag(mats, format="csr"))
    pre = hipla.BlockJacobi(A, blocks)
    for mode in (0, 1):
        got = ritz(A, pre, mode)
        assert len(got) == 1 and abs(got[0] - 1.0) < 1e-12, (mode, got)


def test_reuse_aware_dispatch_order_changes_no_bit(hip_engine):
    """Grid operators beyond ~1e7 rows get a second, dispatch-ordered copy of their row-block descriptors
    (csrc/csr_stream.h: blkdisp): inside every XCD's share the blocks b, b + P, ..., b + (T - 1) P of T grid planes
    run back to back, so that the operand runs of the neighbouring planes are re-read while they are still in the
    XCD's L2.  Only the workgroup -> row block map changes -- forced on here for a small system (T = 3 and 8): the
    period found is the number of row blocks per grid slab, every row block is still visited exactly once (SpMV
    and its dot partials complete), and the fused loops give the bits of the natural order."""
    import hipla
    from minres import MinRes
    from solvers.bramblepasciak_new import BpcgSession
    s = mac_stokes(3, 40, 0.01)
    f, g = s.rhs(0)
    x = np.random.default_rng(1).standard_normal(s.n_u)

    def run(planes, nit=25):
        with hip_engine.overrides(dispatch=(planes, 0, 5 if planes == 8 else 0)):
            A, B = hipla.SparseMatrix.from_scipy(s.A), hipla.SparseMatrix.from_scipy(s.B)
            ya, yb = hipla.Vector(s.n_u), hipla.Vector(s.n_p)
            xv = hipla.Vector.from_numpy(x)
            ya.data = A * xv
            yb.data = B * xv
            preA = hipla.BlockJacobi(A, s.line_blocks(3))
            preS = hipla.DiagonalMatrix(1.0 / s.mass)
            sol = hipla.BlockVector([hipla.Vector(s.n_u), hipla.Vector(s.n_p)])
            with contextlib.redirect_stdout(io.StringIO()):
                ses = BpcgSession(Form(A), Form(B), None, hipla.Vector.from_numpy(f), hipla.Vector.from_numpy(g), preA, preS,
                                  sol=sol)
                ses.first_direction()
                ses.fused.start(ses.wdn, ses.err0, 0.0, True, nit)
                ses.fused.enqueue(0, nit)
                ses.fused.poll()
                K = hipla.BlockMatrix([[A, B.T], [B, None]])
                Cm = hipla.BlockMatrix([[preA, None], [None, preS]])
                u, errors = MinRes(mat=K, pre=Cm, rhs=hipla.BlockVector([hipla.Vector.from_numpy(f), hipla.Vector.from_numpy(g)]),
                                   maxsteps=nit, tol=0.0, printrates=False)
            return dict(ya=ya.numpy(), yb=yb.numpy(), hist=ses.fused.history(nit - 1).copy(), sol=sol.numpy(),
                        minres=np.array(errors), a=A.handle.info(), b=B.handle.info())

    ref = run(0)
    assert ref["a"]["dispatch_period"] == 0.0 and ref["a"]["operand_form"] == "staged"
    np.testing.assert_allclose(ref["ya"], s.A @ x, rtol=1e-13, atol=1e-13)
    for planes in (3, 8):
        got = run(planes)
        rows_per_block = s.n_u / got["a"]["row_blocks"]
        slab = s.velocity_slab_offsets[1] - s.velocity_slab_offsets[0]
        assert got["a"]["dispatch_planes"] == planes
        assert abs(got["a"]["dispatch_period"] - slab / rows_per_block) < 0.05 * slab / rows_per_block + 2
        for key in ("ya", "yb", "hist", "sol", "minres"):
            np.testing.assert_array_equal(got[key], ref[key])
    assert np.all(np.isfinite(ref["hist"]))


@pytest.mark.parametrize("case", ["stokes3d_n10_bjac_minres", "stokes2d_n24_jacobi_minres",
                                  "stokes3d_n5_facet_x12_minres"])
def test_minres_sum_placement_gives_identical_bits(hip_engine, case):
    """The fused MINRES loop evaluates its two dot-product sums either inside the consuming kernels
    (short sums: the launch-bound small systems) or in a stand-alone kernel (long sums) -- the same
    reduction tree, so errors and solution agree bit for bit; and both match the golden."""
    import hipla
    from minres import MinRes
    d = np.load(golden_path(case))
    c, _, A, B, preA, preS = case_operands(d)
    K = hipla.BlockMatrix([[A, B.T], [B, None]])
    Cm = hipla.BlockMatrix([[preA, None], [None, preS]])
    outs = []
    for mode in (1, 0):
        with hip_engine.overrides(minres_fold=mode):
            with contextlib.redirect_stdout(io.StringIO()), fused_loops_counted() as counts:
                u, errors = MinRes(mat=K, pre=Cm, rhs=hipla.BlockVector([hipla.Vector.from_numpy(c.f),
                                                                         hipla.Vector.from_numpy(c.g)]),
                                   maxsteps=int(d["maxsteps"]), tol=float(d["tol"]), printrates=False)
            assert counts["minres"] == 1
            outs.append((np.array(errors), u.numpy()))
    np.testing.assert_array_equal(outs[0][0], outs[1][0])
    np.testing.assert_array_equal(outs[0][1], outs[1][1])
    check_history(outs[0][0], d["errors"], d["window"])
    check_iterations(len(outs[0][0]) - 1, d["iterations"], d)


@pytest.mark.parametrize("case", ["stokes3d_n10_bjac_bpcg1", "stokes2d_n48_jacobi_bpcg1", "stokes2d_n24_bjac_bpcg1",
                                  "stokes3d_n5_facet_x12_bpcg1"])
def test_bpcg1_small_system_form_gives_identical_bits(hip_engine, case):
    """Small systems run the fused textbook BPCG (bramble_pasciak_cg.py:110-143) in 6 dependent launches instead of 10:
    the loop-top bookkeeping (:115-119), alpha (:129) and rho_new / beta (:137-138) are evaluated by every workgroup of
    the consuming kernels (the summation tree of the stand-alone scalar kernel), and the rows of A add their row of
    B^T dp from B^T's fixed-width copy (nss_bpcg1_fold_mode).  Errors and solution agree BIT FOR BIT with the
    10-launch form; both match the golden."""
    import hipla
    from bramble_pasciak_cg import bramble_pasciak_cg
    d = np.load(golden_path(case))
    c, _, A, B, preA, preS = case_operands(d)
    fv, gv = hipla.Vector.from_numpy(c.f), hipla.Vector.from_numpy(c.g)
    outs = {}
    for mode in (0, 1):
        with hip_engine.overrides(bpcg1_fold=mode):
            with contextlib.redirect_stdout(io.StringIO()), fused_loops_counted() as counts:
                sol, errors = bramble_pasciak_cg(A, B, None, preA, preS, fv, gv, tolerance=float(d["tol"]),
                                                 max_steps=int(d["maxsteps"]), print_rates=False)
            assert counts["bpcg1"] == 1
            outs[mode] = (np.array(errors), sol.numpy())
    np.testing.assert_array_equal(outs[1][0], outs[0][0])
    np.testing.assert_array_equal(outs[1][1], outs[0][1])
    check_history(outs[1][0], d["errors"], d["window"])
    check_iterations(len(outs[1][0]) - 1, d["iterations"], d)


@pytest.mark.parametrize("case", ["stokes3d_n10_bjac_minres", "stokes2d_n24_jacobi_minres",
                                  "stokes3d_n5_facet_x12_minres"])
def test_minres_merged_launches_give_identical_bits(hip_engine, case):
    """Launch-bound systems run the fused MINRES iteration (minres.py:96-144) in three dependent launches: the rows of
    A add their row of B^T z1 from a fixed-width copy in the epilogue (B^T of the staggered grids has two entries per
    row) and share the launch with the rows of B (nss_minres_fuse_mode).  Same products, same order of additions as
    the round-2 form: with the block Jacobi kept apart (mode 2) errors and solution agree BIT FOR BIT with mode 0;
    with the block Jacobi inside M3 as well (mode 1, what small systems run) the dot partials are grouped differently
    and the history agrees to rounding; every form matches the golden (plain grids and the facet-block inflation, whose
    B^T keeps two entries per row)."""
    import hipla
    from minres import MinRes
    d = np.load(golden_path(case))
    c, _, A, B, preA, preS = case_operands(d)
    K = hipla.BlockMatrix([[A, B.T], [B, None]])
    Cm = hipla.BlockMatrix([[preA, None], [None, preS]])
    outs = {}
    for mode in (0, 2, 1):
        with hip_engine.overrides(minres_fuse=mode):
            with contextlib.redirect_stdout(io.StringIO()), fused_loops_counted() as counts:
                u, errors = MinRes(mat=K, pre=Cm, rhs=hipla.BlockVector([hipla.Vector.from_numpy(c.f),
                                                                         hipla.Vector.from_numpy(c.g)]),
                                   maxsteps=int(d["maxsteps"]), tol=float(d["tol"]), printrates=False)
            assert counts["minres"] == 1
            outs[mode] = (np.array(errors), u.numpy())
    np.testing.assert_array_equal(outs[2][0], outs[0][0])
    np.testing.assert_array_equal(outs[2][1], outs[0][1])
    w = min(25, len(outs[1][0]), len(outs[0][0]))           # (rounding differences grow along a Krylov history)
    np.testing.assert_allclose(outs[1][0][:w], outs[0][0][:w], rtol=1e-7)
    for mode in (0, 1):
        check_history(outs[mode][0], d["errors"], d["window"])
        check_iterations(len(outs[mode][0]) - 1, d["iterations"], d)


def test_drivers_on_gpu(hip_engine, tmp_path):
    """Harness / driver shape on the product engine: NavierStokes.SolveInitial takes the fused
    loop, run.py writes the reference's CSV columns, stokes_hcurldiv's call converges."""
    import run as harness
    from discretizations import bdm_hybrid
    from stokes_hcurldiv import solve_stokes
    from templates.NavierStokesSIMPLE_iterative import NavierStokes, SyntheticMesh
    ns = NavierStokes(SyntheticMesh(0.125, dim=3), nu=0.001, inflow="inlet", outflow="outlet", wall="wall|cyl",
                      uin=None, timestep=0.002, order=1)
    with contextlib.redirect_stdout(io.StringIO()):
        ns.SolveInitial(iterative=True, GS=False, tol=1e-8)
    s = ns.system
    f, g = s.rhs(0)
    x = np.concatenate([ns.velocity.numpy(), ns.gfup.numpy()])
    assert np.linalg.norm(np.concatenate([f, g]) - s.saddle_matrix() @ x) / np.linalg.norm(f) < 1e-5
    assert ns.stokes_bpcg_iterations > 5 and ns.stokes_bpcg_time > 0
    methods = {"hybrid_dg": {"solve": harness.solve_hybrid, "discretizations": {"HDG BDM 1": bdm_hybrid(1, 10)}}}
    with contextlib.redirect_stdout(io.StringIO()):
        data = harness.run([0.125], methods, harness.solver_factories, str(tmp_path / "errors.csv"), False)
    assert set(data.solver) == {"bramble pasciak cg", "minres"}
    for _, grp in data.groupby("solver"):
        assert grp.error.iloc[0] == 1.0 and grp.error.iloc[-1] < 1e-6
    with contextlib.redirect_stdout(io.StringIO()):
        sol, errors, _ = solve_stokes(maxh=0.2, tolerance=1e-8)
    assert errors[-1] < 1e-8


def test_fused_minres_is_selected_and_agrees_with_protocol_path(hip_engine):
    import hipla
    from hipla import fused
    from minres import MinRes
    for case in ("stokes3d_n10_bjac_minres", "stokes2d_n24_jacobi_minres"):
        d = np.load(golden_path(case))
        s, f, g, A, B, preA, preS = operands(d)
        K = hipla.BlockMatrix([[A, B.T], [B, None]])
        Cm = hipla.BlockMatrix([[preA, None], [None, preS]])
        res = {}
        for mode in ("fused", "protocol"):
            fused.ENABLED = mode == "fused"
            try:
                made = []
                orig = fused.MinresLoop.try_create.__func__

                def spy(cls, *a, **kw):
                    out = orig(cls, *a, **kw)
                    made.append(out is not None)
                    return out

                fused.MinresLoop.try_create = classmethod(spy)
                try:
                    out = io.StringIO()
                    with contextlib.redirect_stdout(out):
                        u, errors = MinRes(mat=K, pre=Cm, rhs=hipla.BlockVector([hipla.Vector.from_numpy(f),
                                                                                 hipla.Vector.from_numpy(g)]),
                                           maxsteps=int(d["maxsteps"]), tol=float(d["tol"]), printrates=False)
                finally:
                    fused.MinresLoop.try_create = classmethod(orig)
                assert made == [mode == "fused"]
                res[mode] = (np.array(errors), u.numpy(), "Warning" in out.getvalue())
            finally:
                fused.ENABLED = True
        w = int(d["window"])
        np.testing.assert_allclose(res["fused"][0][:w], res["protocol"][0][:w], rtol=1e-8)
        check_history(res["fused"][0], d["errors"], d["window"])
        check_iterations(len(res["fused"][0]) - 1, d["iterations"], d)
        assert res["fused"][2] == res["protocol"][2] == bool(d["warned"])
        assert np.linalg.norm(res["fused"][1] - res["protocol"][1]) <= 1e-6 * np.linalg.norm(res["protocol"][1])
        check_solution(res["fused"][1], s, f, g, d)


def test_fused_bpcg1_is_selected_and_agrees_with_protocol_path(hip_engine):
    import hipla
    from hipla import fused
    from bramble_pasciak_cg import bramble_pasciak_cg
    for case in ("stokes3d_n10_bjac_bpcg1", "stokes2d_n24_jacobi_bpcg1"):
        d = np.load(golden_path(case))
        s, f, g, A, B, preA, preS = operands(d)
        res = {}
        for mode in ("fused", "protocol"):
            fused.ENABLED = mode == "fused"
            made = []
            orig = fused.Bpcg1Loop.try_create.__func__

            def spy(cls, *a, **kw):
                out = orig(cls, *a, **kw)
                made.append(out is not None)
                return out

            fused.Bpcg1Loop.try_create = classmethod(spy)
            try:
                with contextlib.redirect_stdout(io.StringIO()):
                    x, errors = bramble_pasciak_cg(A, B, None, preA, preS, hipla.Vector.from_numpy(f),
                                                   hipla.Vector.from_numpy(g), tolerance=float(d["tol"]),
                                                   max_steps=int(d["maxsteps"]), print_rates=False)
            finally:
                fused.Bpcg1Loop.try_create = classmethod(orig)
                fused.ENABLED = True
            assert made == [mode == "fused"]
            res[mode] = (np.array(errors), x.numpy())
        w = int(d["window"])
        np.testing.assert_allclose(res["fused"][0][:w], res["protocol"][0][:w], rtol=1e-8)
        check_history(res["fused"][0], d["errors"], d["window"])
        check_iterations(len(res["fused"][0]) - 1, d["iterations"], d)
        assert np.linalg.norm(res["fused"][1] - res["protocol"][1]) <= 1e-6 * np.linalg.norm(res["protocol"][1])
        check_solution(res["fused"][1], s, f, g, d)


def test_fused_bpcg2_breakdown_raises_like_the_reference(hip_engine):
    """<s, K^ s> == 0 makes the reference's `alpha = wd / as_s` raise ZeroDivisionError
    (solvers/bramblepasciak_new.py:226); the fused loop freezes and the host raises the same."""
    import hipla
    from solvers.bramblepasciak_new import BpcgSession
    d = np.load(golden_path("stokes2d_n12_jacobi_bpcg2"))
    s, f, g, A, B, preA, preS = operands(d)
    sol = hipla.BlockVector([hipla.Vector(s.n_u), hipla.Vector(s.n_p)])
    with contextlib.redirect_stdout(io.StringIO()):
        ses = BpcgSession(Form(A), Form(B), None, hipla.Vector.from_numpy(f), hipla.Vector.from_numpy(g), preA, preS,
                          sol=sol)
    ses.s[0][:] = 0.0                 # direction s = 0  ->  <s, K^ s> = 0 in the first iteration
    ses.s[1][:] = 0.0
    ses.first_direction()
    with pytest.raises(ZeroDivisionError):
        ses.fused.run(ses.wdn, ses.err0, 1e-8, True, 50)
    assert np.all(sol.numpy() == 0.0)           # state frozen before any update


def test_fused_loops_with_block_gauss_seidel_preconditioner(hip_engine):
    """Scope row N1 on the hot path: the symmetric multicolour block Gauss-Seidel sweep as preA in
    the three fused loops, against the oracle loops driven by the *sequential* sweep over the
    same block order; and the reference's default `SolveInitial()` (GS=True) end to end."""
    import hipla
    from bramble_pasciak_cg import bramble_pasciak_cg
    from minres import MinRes
    from oracle import krylov_ref as kr
    from solvers.bramblepasciak_new import BpcgSession, BramblePasciakCG
    s = mac_stokes(3, 6, 0.01)
    f, g = s.rhs(0)
    A, B = hipla.SparseMatrix.from_scipy(s.A), hipla.SparseMatrix.from_scipy(s.B)
    G = hipla.BlockGaussSeidel(A, s.line_blocks(3))
    preS = hipla.DiagonalMatrix(1.0 / s.mass)
    pa, ps = kr.symmetric_block_gauss_seidel(s.A, G.idx_host), kr.diag_inverse(s.mass)
    fv, gv = hipla.Vector.from_numpy(f), hipla.Vector.from_numpy(g)
    b = np.concatenate([f, g])
    K = s.saddle_matrix()

    sol = hipla.BlockVector([hipla.Vector(s.n_u), hipla.Vector(s.n_p)])
    with contextlib.redirect_stdout(io.StringIO()):
        ses = BpcgSession(Form(A), Form(B), None, fv, gv, G, preS, sol=sol)
    assert ses.fused is not None
    out = io.StringIO()
    sol = hipla.BlockVector([hipla.Vector(s.n_u), hipla.Vector(s.n_p)])
    with contextlib.redirect_stdout(out):
        it, _ = BramblePasciakCG(Form(A), Form(B), None, fv, gv, G, preS, sol, tol=1e-9, maxsteps=2000)
    hist = np.array([float(m) for m in re.findall(r"it =\s+\d+\s+err =\s+(\S+)", out.getvalue())])
    k = kr.scale_factor(kr.lanczos_ritz(s.A, pa, tol=1e-3))
    assert abs(k - ses.k) < 1e-8 * k
    it_ref, u, p, hist_ref, err0 = kr.bpcg_v2(s.A, s.B, pa, ps, f, g, k, tol=1e-9, maxsteps=2000)
    np.testing.assert_allclose(hist[:25], hist_ref[:25], rtol=1e-8)
    assert abs(it - it_ref) <= max(3, int(0.03 * it_ref))
    assert np.linalg.norm(b - K @ sol.numpy()) < 1e-6 * np.linalg.norm(b)

    with contextlib.redirect_stdout(io.StringIO()):
        x1, errors = bramble_pasciak_cg(A, B, None, G, preS, fv, gv, tolerance=1e-9, max_steps=2000, print_rates=False)
    u1, p1, e_ref, _ = kr.bpcg_v1(s.A, s.B, pa, ps, f, g, kr.scale_factor(kr.lanczos_ritz(s.A, pa, tol=1e-10)),
                                  tolerance=1e-9, max_steps=2000)
    np.testing.assert_allclose(errors[:25], e_ref[:25], rtol=1e-8)
    assert abs(len(errors) - len(e_ref)) <= max(3, int(0.03 * len(e_ref)))

    Km = hipla.BlockMatrix([[A, B.T], [B, None]])
    Cm = hipla.BlockMatrix([[G, None], [None, preS]])
    with contextlib.redirect_stdout(io.StringIO()):
        um, errs = MinRes(mat=Km, pre=Cm, rhs=hipla.BlockVector([fv, gv]), maxsteps=2000, tol=1e-9, printrates=False)
    _, _, m_ref, _ = kr.minres(s.A, s.B, pa, ps, f, g, maxsteps=2000, tol=1e-9)
    np.testing.assert_allclose(errs[:40], m_ref[:40], rtol=1e-8)
    assert np.linalg.norm(b - K @ um.numpy()) < 1e-6 * np.linalg.norm(b)

    # the reference's default driver call: SolveInitial() with GS=True needs fewer iterations
    from templates.NavierStokesSIMPLE_iterative import NavierStokes, SyntheticMesh
    counts = {}
    for gs in (True, False):
        ns = NavierStokes(SyntheticMesh(0.125, dim=3), nu=0.001, inflow="inlet", outflow="outlet", wall="wall|cyl",
                          uin=None, timestep=0.002, order=1)
        with contextlib.redirect_stdout(io.StringIO()):
            ns.SolveInitial(iterative=True, GS=gs, tol=1e-8)
        counts[gs] = ns.stokes_bpcg_iterations
    assert 3 < counts[True] <= counts[False]


def test_static_condensation_path_on_gpu(hip_engine):
    """Scope row N2 on the product engine: `blfA.condense = True`.  The fused loop multiplies with
    the explicit product (I - H^T)(S + A_ii)(I - H) (device SpGEMM) and applies
    harmonic_extension() as its preconditioner step; the statement-by-statement protocol path
    (composite operator, as the reference evaluates it) and the numpy checker engine give the same
    history, and the solve agrees with the uncondensed one."""
    import hipla
    from hipla import fused
    from oracle.numpy_engine import NumpyEngine
    from discretizations import AssembledForm, CondensedForm
    from solvers.bramblepasciak_new import BpcgSession, BramblePasciakCG
    s = mac_stokes(3, 8, 0.01)
    f, g = s.rhs(0)
    b = np.concatenate([f, g])

    def run(eng, pre_kind):
        prev = hipla.set_engine(eng)
        try:
            blfA, blfB = CondensedForm(s), AssembledForm(hipla.SparseMatrix.from_scipy(s.B))
            preM = hipla.DiagonalMatrix(1.0 / s.mass)
            if pre_kind == "jacobi":
                preA = blfA.jacobi()
            else:                                                # blocks of coupling dofs only (S is zero elsewhere)
                idx = s.line_blocks(3).copy()
                idx[(idx >= 0) & blfA.interior[np.maximum(idx, 0)]] = -1
                idx = -np.sort(-idx, axis=0)                     # padding last
                preA = hipla.BlockJacobi(blfA.mat, np.ascontiguousarray(idx[:, (idx >= 0).any(axis=0)]))
            if eng is hip_engine and fused.ENABLED:
                with contextlib.redirect_stdout(io.StringIO()):
                    ses = BpcgSession(blfA, blfB, None, hipla.Vector.from_numpy(f), hipla.Vector.from_numpy(g), preA,
                                      preM)
                assert ses.fused is not None                     # condensed form takes the device-resident loop
                expl = ses.fused.keep[0].to_scipy()
                assert abs(expl - s.A).max() <= 1e-12 * abs(s.A).max()
            sol = hipla.BlockVector([hipla.Vector(s.n_u), hipla.Vector(s.n_p)])
            out = io.StringIO()
            with contextlib.redirect_stdout(out):
                it, _ = BramblePasciakCG(blfA, blfB, None, hipla.Vector.from_numpy(f), hipla.Vector.from_numpy(g),
                                         preA, preM, sol, tol=1e-9, maxsteps=5000)
            hist = np.array([float(m) for m in re.findall(r"it =\s+\d+\s+err =\s+(\S+)", out.getvalue())])
            return it, hist, sol.numpy()
        finally:
            hipla.set_engine(prev)

    for pre_kind in ("jacobi", "bjac"):
        res = {"fused": run(hip_engine, pre_kind)}
        fused.ENABLED = False
        try:
            res["protocol"] = run(hip_engine, pre_kind)
        finally:
            fused.ENABLED = True
        res["numpy"] = run(NumpyEngine(), pre_kind)
        it_f, hist_f, x = res["fused"]
        for other in ("protocol", "numpy"):
            it_o, hist_o, x_o = res[other]
            w = min(30, len(hist_f), len(hist_o))
            np.testing.assert_allclose(hist_f[:w], hist_o[:w], rtol=1e-8)
            assert abs(it_f - it_o) <= max(3, int(0.03 * it_o))
            assert np.linalg.norm(x - x_o) < 1e-5 * np.linalg.norm(x_o)
        assert np.linalg.norm(b - s.saddle_matrix() @ x) < 1e-5 * np.linalg.norm(b)
        assert 5 < it_f < 5000
    A = hipla.SparseMatrix.from_scipy(s.A)
    ref = hipla.BlockVector([hipla.Vector(s.n_u), hipla.Vector(s.n_p)])
    with contextlib.redirect_stdout(io.StringIO()):
        BramblePasciakCG(AssembledForm(A), AssembledForm(hipla.SparseMatrix.from_scipy(s.B)), None,
                         hipla.Vector.from_numpy(f), hipla.Vector.from_numpy(g), hipla.JacobiPreconditioner(A),
                         hipla.DiagonalMatrix(1.0 / s.mass), ref, tol=1e-9, maxsteps=5000)
    xr = ref.numpy()
    assert np.linalg.norm(x[:s.n_u] - xr[:s.n_u]) < 1e-5 * np.linalg.norm(xr[:s.n_u])


def test_heat_config1_driver(hip_engine):
    """BASELINE config 1 through the package's heat.py: CG history and Galerkin spectrum against the
    golden produced with the reference's orthonormalization.py."""
    import heat
    d = np.load(__import__("conftest").golden_path("cfg1_heat_plumbing"))
    x, hist, gal = heat.solve(n=int(d["n"]), seed=int(d["seed"]))
    assert len(hist) - 1 == int(d["cg_iterations"])
    np.testing.assert_allclose(hist, d["cg_history"], rtol=1e-8)
    assert abs(np.linalg.norm(x.numpy()) - float(d["cg_x_norm"])) < 1e-9 * float(d["cg_x_norm"])
    np.testing.assert_allclose(np.linalg.eigvalsh(gal), np.linalg.eigvalsh(d["galerkin"]), rtol=1e-7)


def test_amg_vcycle_and_fused_bpcg_with_amg(hip_engine):
    """Scope row N3: the smoothed-aggregation V(1,1)-cycle on the device against the identical
    cycle on the identical hierarchy run by the numpy checker engine; the fused BPCG loop with
    preA = AMG and with the additive MypreA form AMG + block Jacobi (:383) against the protocol loop
    on the checker engine; mesh-independent iteration counts."""
    import hipla
    from oracle.numpy_engine import NumpyEngine
    from solvers.bramblepasciak_new import BpcgSession, BramblePasciakCG
    results = {}
    for n in (12, 20):
        s = mac_stokes(3, n, 0.01)
        f, g = s.rhs(0)
        x = np.random.default_rng(n).standard_normal(s.n_u)
        per_engine = {}
        for name in ("hip", "numpy"):
            eng = hip_engine if name == "hip" else NumpyEngine()
            prev = hipla.set_engine(eng)
            try:
                A, B = hipla.SparseMatrix.from_scipy(s.A), hipla.SparseMatrix.from_scipy(s.B)
                V = hipla.SmoothedAggregationAMG(A, coarse_size=300)
                J = hipla.BlockJacobi(A, s.line_blocks(3))
                preS = hipla.DiagonalMatrix(1.0 / s.mass)
                y = hipla.Vector(s.n_u)
                y.data = V * hipla.Vector.from_numpy(x)
                y2 = hipla.Vector(s.n_u)
                y2.data = 1.5 * V * hipla.Vector.from_numpy(x)
                runs = {}
                for label, pre in (("amg", V), ("amg+bjac", V + J), ("amg+jacobi", V + hipla.JacobiPreconditioner(A))):
                    sol = hipla.BlockVector([hipla.Vector(s.n_u), hipla.Vector(s.n_p)])
                    if name == "hip":
                        with contextlib.redirect_stdout(io.StringIO()):
                            ses = BpcgSession(Form(A), Form(B), None, hipla.Vector.from_numpy(f),
                                              hipla.Vector.from_numpy(g), pre, preS, sol=sol)
                        assert ses.fused is not None            # native: takes the device-resident loop
                        sol = hipla.BlockVector([hipla.Vector(s.n_u), hipla.Vector(s.n_p)])
                    out = io.StringIO()
                    with contextlib.redirect_stdout(out):
                        it, _ = BramblePasciakCG(Form(A), Form(B), None, hipla.Vector.from_numpy(f),
                                                 hipla.Vector.from_numpy(g), pre, preS, sol, tol=1e-9, maxsteps=2000)
                    hist = np.array([float(m) for m in re.findall(r"it =\s+\d+\s+err =\s+(\S+)", out.getvalue())])
                    runs[label] = (it, hist, sol.numpy())
                per_engine[name] = (V.level_sizes, y.numpy(), y2.numpy(), runs)
            finally:
                hipla.set_engine(prev)
        (lv_h, y_h, y2_h, runs_h), (lv_n, y_n, y2_n, runs_n) = per_engine["hip"], per_engine["numpy"]
        assert lv_h == lv_n and len(lv_h) >= 2
        assert np.linalg.norm(y_h - y_n) <= 1e-12 * np.linalg.norm(y_n)
        assert np.linalg.norm(y2_h - 1.5 * y_n) <= 1e-12 * np.linalg.norm(y_n)
        b = np.concatenate([f, g])
        for label in ("amg", "amg+bjac", "amg+jacobi"):
            it_h, hist_h, x_h = runs_h[label]
            it_n, hist_n, x_n = runs_n[label]
            np.testing.assert_allclose(hist_h[:25], hist_n[:25], rtol=1e-8)
            assert abs(it_h - it_n) <= max(3, int(0.03 * it_n))
            assert np.linalg.norm(b - s.saddle_matrix() @ x_h) < 1e-6 * np.linalg.norm(b)
        results[n] = runs_h["amg"][0]
    assert results[20] < 1.5 * results[12] + 10           # iteration count nearly mesh-independent


def test_auxiliary_space_mypre_a_native_in_the_fused_loop(hip_engine):
    """Scope row N3 as the reference composes it (templates/NavierStokesSIMPLE_iterative.py:208-391):
    MypreA = block smoother + `transform @ preAh1 @ transform.T`, additive (GS=False, :383) and
    multiplicative (GS=True, :376-381).  Both are applied natively inside the fused BPCG loop (one
    nss_amg_create_auxiliary handle; the multiplicative form = sweep, residual, correction, back sweep);
    history and solution agree with the statement-by-statement protocol path on the GPU and with the
    numpy checker engine; plain and facet-block (inflated) systems; also inside fused MINRES / BPCG v1
    (additive form)."""
    import hipla
    from hipla import fused
    from oracle.numpy_engine import NumpyEngine
    from bramble_pasciak_cg import bramble_pasciak_cg
    from minres import MinRes
    from solvers.bramblepasciak_new import BramblePasciakCG
    from templates.NavierStokesSIMPLE_iterative import MypreA, auxiliary_space_preconditioner

    def run(eng, s, blocks, gs, solver="bpcg2"):
        prev = hipla.set_engine(eng)
        try:
            f, g = s.rhs(0)
            A, B = hipla.SparseMatrix.from_scipy(s.A), hipla.SparseMatrix.from_scipy(s.B)
            _, _, aux = auxiliary_space_preconditioner(s)
            preA = MypreA(None, Form(A), blocks, GS=gs, aux=aux)
            preS = hipla.DiagonalMatrix(1.0 / s.mass)
            fv, gv = hipla.Vector.from_numpy(f), hipla.Vector.from_numpy(g)
            out = io.StringIO()
            with contextlib.redirect_stdout(out), fused_loops_counted() as counts:
                if solver == "bpcg2":
                    sol = hipla.BlockVector([hipla.Vector(s.n_u), hipla.Vector(s.n_p)])
                    it, _ = BramblePasciakCG(Form(A), Form(B), None, fv, gv, preA, preS, sol, tol=1e-9, maxsteps=3000)
                    hist = np.array([float(m) for m in re.findall(r"it =\s+\d+\s+err =\s+(\S+)", out.getvalue())])
                elif solver == "bpcg1":
                    sol, hist = bramble_pasciak_cg(A, B, None, preA, preS, fv, gv, tolerance=1e-9, max_steps=3000,
                                                   print_rates=False)
                    it = len(hist) - 1
                else:
                    K = hipla.BlockMatrix([[A, B.T], [B, None]])
                    Cm = hipla.BlockMatrix([[preA, None], [None, preS]])
                    sol, hist = MinRes(mat=K, pre=Cm, rhs=hipla.BlockVector([fv, gv]), maxsteps=3000, tol=1e-9,
                                       printrates=False)
                    it = len(hist) - 1
            return it, np.array(hist), sol.numpy(), counts[solver]
        finally:
            hipla.set_engine(prev)

    plain = mac_stokes(3, 10, 0.01)
    facet = mac_stokes(2, 12, 0.01).inflate(5)
    cases = [(plain, plain.line_blocks(3), False, "bpcg2"), (plain, plain.line_blocks(3), True, "bpcg2"),
             (facet, facet.line_blocks(1), False, "bpcg2"), (facet, facet.line_blocks(1), True, "bpcg2"),
             (plain, plain.line_blocks(3), False, "minres"), (plain, plain.line_blocks(3), False, "bpcg1")]
    for s, blocks, gs, solver in cases:
        it_f, hist_f, x_f, used = run(hip_engine, s, blocks, gs, solver)
        assert used == 1, "fused %s loop not taken (GS=%s)" % (solver, gs)
        fused.ENABLED = False
        try:
            it_p, hist_p, x_p, used_p = run(hip_engine, s, blocks, gs, solver)
        finally:
            fused.ENABLED = True
        assert used_p == 0
        it_n, hist_n, x_n, _ = run(NumpyEngine(), s, blocks, gs, solver)
        f, g = s.rhs(0)
        b = np.concatenate([f, g])
        for it_o, hist_o, x_o in ((it_p, hist_p, x_p), (it_n, hist_n, x_n)):
            w = min(20, len(hist_f), len(hist_o))
            np.testing.assert_allclose(hist_f[:w], hist_o[:w], rtol=1e-8)
            assert abs(it_f - it_o) <= max(3, int(0.05 * it_o))
            assert np.linalg.norm(x_f - x_o) < 1e-5 * np.linalg.norm(x_o)
        assert np.linalg.norm(b - s.saddle_matrix() @ x_f) < 1e-6 * np.linalg.norm(b)
        assert 3 < it_f < 400


def test_fused_minres_and_bpcg1_with_amg(hip_engine):
    """preA = AMG and the additive AMG + block Jacobi inside the fused MINRES and BPCG-v1 loops
    (`pre_amg` of nss_minres_t / nss_bpcg1_t): the fused loop is selected and its history agrees
    with the statement-by-statement protocol path on the GPU and with the numpy checker engine."""
    import hipla
    from hipla import fused
    from oracle.numpy_engine import NumpyEngine
    from bramble_pasciak_cg import bramble_pasciak_cg
    from minres import MinRes
    s = mac_stokes(3, 12, 0.01)
    f, g = s.rhs(0)
    b = np.concatenate([f, g])

    def solve(kind, label, eng):
        prev = hipla.set_engine(eng)
        try:
            A, B = hipla.SparseMatrix.from_scipy(s.A), hipla.SparseMatrix.from_scipy(s.B)
            V = hipla.SmoothedAggregationAMG(A, coarse_size=300)
            preA = V if label == "amg" else V + hipla.BlockJacobi(A, s.line_blocks(3))
            preS = hipla.DiagonalMatrix(1.0 / s.mass)
            fv, gv = hipla.Vector.from_numpy(f), hipla.Vector.from_numpy(g)
            with contextlib.redirect_stdout(io.StringIO()):
                if kind == "minres":
                    K = hipla.BlockMatrix([[A, B.T], [B, None]])
                    Cm = hipla.BlockMatrix([[preA, None], [None, preS]])
                    x, errors = MinRes(mat=K, pre=Cm, rhs=hipla.BlockVector([fv, gv]), maxsteps=2000, tol=1e-9,
                                       printrates=False)
                else:
                    x, errors = bramble_pasciak_cg(A, B, None, preA, preS, fv, gv, tolerance=1e-9, max_steps=2000,
                                                   print_rates=False)
            return np.array(errors), x.numpy()
        finally:
            hipla.set_engine(prev)

    for kind, loop in (("minres", fused.MinresLoop), ("bpcg1", fused.Bpcg1Loop)):
        for label in ("amg", "amg+bjac"):
            res = {}
            for mode in ("fused", "protocol"):
                fused.ENABLED = mode == "fused"
                made = []
                orig = loop.try_create.__func__

                def spy(cls, *a, _orig=orig, _made=made, **kw):
                    out = _orig(cls, *a, **kw)
                    _made.append(out is not None)
                    return out

                loop.try_create = classmethod(spy)
                try:
                    res[mode] = solve(kind, label, hip_engine)
                finally:
                    loop.try_create = classmethod(orig)
                    fused.ENABLED = True
                assert made == [mode == "fused"], (kind, label, mode, made)
            res["numpy"] = solve(kind, label, NumpyEngine())
            n_f, n_p, n_n = (len(res[m][0]) for m in ("fused", "protocol", "numpy"))
            assert abs(n_f - n_n) <= max(3, int(0.03 * n_n)) and abs(n_f - n_p) <= max(3, int(0.03 * n_p))
            w = min(25, n_f, n_n, n_p)
            np.testing.assert_allclose(res["fused"][0][:w], res["numpy"][0][:w], rtol=1e-8)
            np.testing.assert_allclose(res["fused"][0][:w], res["protocol"][0][:w], rtol=1e-8)
            assert np.linalg.norm(b - s.saddle_matrix() @ res["fused"][1]) < 1e-6 * np.linalg.norm(b)
            assert n_f < 250                                   # AMG-preconditioned: far below the Jacobi counts


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_fused_loops_on_unstructured_saddle_systems(hip_engine, seed):
    """Nothing in the fused loops knows about the MAC grid: random sparse SPD `A` with scattered
    columns, random full-row-rank `B`, ragged rows and empty rows in
    B^T; BPCG v2, BPCG v1 and MINRES against the oracle restatements on the same operands."""
    import scipy.sparse as sp
    import hipla
    from oracle import krylov_ref as kr
    from bramble_pasciak_cg import bramble_pasciak_cg
    from minres import MinRes
    from solvers.bramblepasciak_new import BramblePasciakCG
    rng = np.random.default_rng(100 + seed)
    n_u, n_p = 2500 + 300 * seed, 600 + 50 * seed
    G = sp.random(n_u, n_u, density=4.0 / n_u, random_state=np.random.RandomState(seed), data_rvs=rng.standard_normal)
    A = (G @ G.T + sp.diags(1.0 + rng.random(n_u))).tocsr()
    A.sort_indices()
    B = sp.random(n_p, n_u, density=5.0 / n_u, random_state=np.random.RandomState(seed + 7),
                  data_rvs=rng.standard_normal).tolil()
    for r in range(n_p):                                   # full row rank: a private column per row
        B[r, r * (n_u // n_p)] = 2.0 + rng.random()
    B = B.tocsr()
    B.sort_indices()
    assert np.diff(B.T.tocsr().indptr).min() == 0          # B^T has empty rows
    f, g = rng.standard_normal(n_u), rng.standard_normal(n_p)
    mass = 0.5 + rng.random(n_p)
    Ad, Bd = hipla.SparseMatrix.from_scipy(A), hipla.SparseMatrix.from_scipy(B)
    preA, preS = hipla.JacobiPreconditioner(Ad), hipla.DiagonalMatrix(1.0 / mass)
    pa, ps = kr.jacobi(A), kr.diag_inverse(mass)
    K = sp.bmat([[A, B.T], [B, None]], format="csr")
    b = np.concatenate([f, g])
    tol, maxsteps = 1e-9, 4000

    # BPCG v2
    sol = hipla.BlockVector([hipla.Vector(n_u), hipla.Vector(n_p)])
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        it, _ = BramblePasciakCG(Form(Ad), Form(Bd), None, hipla.Vector.from_numpy(f), hipla.Vector.from_numpy(g), preA,
                                 preS, sol, tol=tol, maxsteps=maxsteps)
    hist = np.array([float(m) for m in re.findall(r"it =\s+\d+\s+err =\s+(\S+)", out.getvalue())])
    from solvers.bramblepasciak_new import BpcgSession
    with contextlib.redirect_stdout(io.StringIO()):
        ses = BpcgSession(Form(Ad), Form(Bd), None, hipla.Vector.from_numpy(f), hipla.Vector.from_numpy(g), preA, preS)
    assert ses.fused is not None
    it_o, u_o, p_o, hist_o = kr.bpcg_v2(A, B, pa, ps, f, g, ses.k, tol=tol, maxsteps=maxsteps)[:4]
    # (no stable window is recorded for these random systems; measured: a regrouping of the dot partials -- B planned
    # with shorter row blocks -- moves entry 20 of seed 1 by 1.6e-8: 1e-8 over the first 15 entries, 1e-6 over 25)
    w = min(15, len(hist), len(hist_o))
    np.testing.assert_allclose(hist[:w], hist_o[:w], rtol=1e-8)
    w = min(25, len(hist), len(hist_o))
    np.testing.assert_allclose(hist[:w], hist_o[:w], rtol=1e-6)
    assert abs(it - it_o) <= max(3, int(0.03 * it_o))
    assert np.linalg.norm(b - K @ sol.numpy()) < 1e-6 * np.linalg.norm(b)

    # BPCG v1 and MINRES: converge to the same solution as the oracle, same iteration counts
    out1 = io.StringIO()
    with contextlib.redirect_stdout(out1):
        x1, errs1 = bramble_pasciak_cg(Ad, Bd, None, preA, preS, hipla.Vector.from_numpy(f), hipla.Vector.from_numpy(g),
                                       tolerance=tol, max_steps=maxsteps, print_rates=False)
    with contextlib.redirect_stdout(io.StringIO()):
        um, errsm = MinRes(mat=hipla.BlockMatrix([[Ad, Bd.T], [Bd, None]]),
                           pre=hipla.BlockMatrix([[preA, None], [None, preS]]),
                           rhs=hipla.BlockVector([hipla.Vector.from_numpy(f), hipla.Vector.from_numpy(g)]),
                           maxsteps=maxsteps, tol=tol, printrates=False)
    assert errs1[-1] < tol and len(errs1) < maxsteps
    # v1 estimates its own scale factor (tol 1e-10 Lanczos, :70-71) and prints it: the oracle takes that k
    k1 = float(re.search(r"scale factor:\s+(\S+)", out1.getvalue()).group(1))
    errs1_o = kr.bpcg_v1(A, B, pa, ps, f, g, k1, tolerance=tol, max_steps=maxsteps)[2]
    w1 = min(15, len(errs1), len(errs1_o))        # random operands: the history separates early (1.3e-8 at entry 20)
    np.testing.assert_allclose(np.array(errs1)[:w1], np.array(errs1_o)[:w1], rtol=1e-8)
    assert abs(len(errs1) - len(errs1_o)) <= max(3, int(0.03 * len(errs1_o)))
    for x in (x1.numpy(), um.numpy()):
        assert np.linalg.norm(b - K @ x) < 1e-6 * np.linalg.norm(b)
        assert np.linalg.norm(x - sol.numpy()) < 1e-5 * np.linalg.norm(sol.numpy())
    errs_o = kr.minres(A, B, pa, ps, f, g, maxsteps=maxsteps, tol=tol)[2]
    w = min(25, len(errsm), len(errs_o))
    np.testing.assert_allclose(np.array(errsm)[:w], np.array(errs_o)[:w], rtol=1e-8)


def test_time_stepping_on_gpu(hip_engine):
    """Scope row N4 on the product engine against the oracle's statement-by-statement `do_time_step`
    (templates/NavierStokesSIMPLE_iterative.py:424-443; direct sparse solves): with the inner CG solves run to
    convergence DoTimeStep's right-hand side, its unprojected increment, the projected increment and the new
    velocity agree to 1e-8; with the reference's inner precision (CGSolver(..., precision=1e-4), :92) the step
    agrees to that precision; Project leaves a discretely divergence-free field."""
    import hipla
    from templates.NavierStokesSIMPLE_iterative import NavierStokes, SyntheticMesh

    def fresh():
        ns = NavierStokes(SyntheticMesh(0.1, dim=3), nu=0.01, inflow="inlet", outflow="outlet", wall="wall|cyl", uin=None,
                          timestep=0.05, order=1)
        ns.AddForce(np.random.default_rng(8).standard_normal(ns.system.n_u))
        return ns

    ns = fresh()
    s = ns.system
    m_u = np.full(s.n_u, s.h ** s.dim)
    v0 = np.random.default_rng(2).standard_normal(s.n_u)
    vel = hipla.Vector.from_numpy(v0)
    ns.Project(vel)
    assert np.linalg.norm(s.B @ vel.numpy()) < 1e-6 * np.linalg.norm(s.B @ v0)
    ref_v, _ = kr.project(s.B, m_u, v0)
    assert np.linalg.norm(vel.numpy() - ref_v) < 1e-6 * np.linalg.norm(ref_v)      # invproj: CG to 1e-8 (:130)
    u0 = ref_v
    cops = s.convection_operators()
    want = kr.do_time_step(s.A, s.B, m_u, ns.timestep, u0, ns.f.vec.numpy(), lambda u: kr.upwind_convection(cops, u))

    def rel(a, b):
        return np.linalg.norm(a - b) / np.linalg.norm(b)

    # (i) the reference's inner precision: agreement to that precision
    ns.gfu.data = hipla.Vector.from_numpy(u0)
    with contextlib.redirect_stdout(io.StringIO()):
        ns.DoTimeStep()
    assert rel(ns.gfu.numpy(), want["u"]) < 1e-4
    assert np.linalg.norm(s.B @ ns.gfu.numpy()) < 1e-5 * np.linalg.norm(ns.gfu.numpy()) * abs(s.B).max()
    # (ii) inner solves run to convergence: every stage of the step against the oracle
    ns = fresh()
    ops = ns._time_stepping_operators()
    ops["invmstar"] = hipla.CGSolver(ops["mstar"], pre=hipla.JacobiPreconditioner(ops["mstar"]), precision=1e-14, maxsteps=5000)
    ops["invproj"] = hipla.CGSolver(ops["Lp"], pre=hipla.JacobiPreconditioner(ops["Lp"]), precision=1e-14, maxsteps=20000)
    ns.gfu.data = hipla.Vector.from_numpy(u0)
    temp = ns.a.mat.CreateColVector()
    temp.data = ns.conv_operator * ns.gfu                  # :429-431, the statements of DoTimeStep
    temp.data += ns.f.vec
    temp.data += -ns.a.mat * ns.gfu
    assert rel(temp.numpy(), want["temp"]) < 1e-13
    raw = ns.a.mat.CreateColVector()
    raw.data = ops["invmstar"] * temp                      # :433
    assert rel(raw.numpy(), want["temp2_unprojected"]) < 1e-9
    proj = raw.CreateVector()
    proj.data = raw
    ns.Project(proj)                                        # :434
    assert rel(proj.numpy(), want["temp2"]) < 1e-8
    with contextlib.redirect_stdout(io.StringIO()):
        ns.DoTimeStep()
    assert rel(ns.gfu.numpy(), want["u"]) < 1e-8
    assert rel((ns.gfu.numpy() - u0) / ns.timestep, want["temp2"]) < 1e-8


def test_mypre_a_mult_against_the_oracle(hip_engine):
    """`MypreA.Mult` on the GPU (multicolour sweeps, native auxiliary-space handle) against the oracle's
    statement-by-statement `kr.mypre_a` (templates/NavierStokesSIMPLE_iterative.py:375-383; SEQUENTIAL sweeps in
    the GPU's colour-major block order), 1e-12: (i) with exact component solves the auxiliary term of the oracle
    is built from sparse LU factorisations of the component Laplacians -- nothing of the product; (ii) with the
    product's V-cycles the oracle takes the GPU's auxiliary apply as a black box, which pins the order of the five
    statements of the multiplicative form."""
    import hipla
    from templates.NavierStokesSIMPLE_iterative import MypreA, auxiliary_space_preconditioner

    def gpu_apply(op, x, n):
        y = hipla.Vector(n)
        op.Mult(hipla.Vector.from_numpy(x), y)
        return y.numpy()

    for s, blocks in ((mac_stokes(3, 7, 0.01), None), (mac_stokes(2, 10, 0.01).inflate(5), "facet")):
        blocks = s.line_blocks(3) if blocks is None else s.line_blocks(1)
        A = hipla.SparseMatrix.from_scipy(s.A)
        space = s.auxiliary_space()
        x = np.random.default_rng(12).standard_normal(s.n_u)
        # (i) exact component solves on both sides
        transform = hipla.SparseMatrix.from_scipy(space["transform"])
        comps = [hipla.SmoothedAggregationAMG(hipla.SparseMatrix.from_scipy(lap), coarse_size=10 ** 9)
                 for lap in space["laplacians"]]
        assert all(len(c.level_sizes) == 1 for c in comps)
        aux_gpu = hipla.AuxiliarySpaceAMG(transform, comps)
        aux_ref = kr.auxiliary_space_term(space["transform"], space["laplacians"], space["ranges"])
        ya = gpu_apply(aux_gpu, x, s.n_u)
        assert np.linalg.norm(ya - aux_ref(x)) < 1e-11 * np.linalg.norm(ya)
        # (ii) the product's V-cycles, applied as a black box inside the oracle's composition
        _, _, aux_cycles = auxiliary_space_preconditioner(s)
        for aux, ref_aux, tol in ((aux_gpu, aux_ref, 1e-11), (aux_cycles, lambda r: gpu_apply(aux_cycles, r, s.n_u), 1e-12)):
            for gs in (True, False):
                op = MypreA(None, Form(A), blocks, GS=gs, aux=aux)
                order = op.idx_host if gs else blocks            # the sweep's colour-major block order
                want = kr.mypre_a(s.A, order, ref_aux, gs)(x)
                got = gpu_apply(op, x, s.n_u)
                assert np.linalg.norm(got - want) < tol * np.linalg.norm(want), (s.n_u, gs, tol)


def test_components_sharing_a_hierarchy_are_cycled_together(hip_engine):
    """The auxiliary-space term `T (sum_c E_c V_c E_c^T) T^T` (templates/NavierStokesSIMPLE_iterative.py:336-337,357,
    380,383): components whose Laplacians are the same matrix share one hierarchy and are cycled TOGETHER -- every
    level operator read once for all right-hand sides (csrc/amg.hip: csr_multi_kernel, interleaved work vectors) --
    instead of one V-cycle after the other.  Same cycle, another summation order inside a row: 1e-13 against the
    component-by-component form, 2 and 3 components, several levels, plain and accumulating applies, inside the fused
    BPCG loop with MypreA(GS=True)."""
    import hipla
    from solvers.bramblepasciak_new import BpcgSession
    from templates.NavierStokesSIMPLE_iterative import MypreA, auxiliary_space_preconditioner
    for dim, n, min_levels in ((2, 300, 3), (3, 40, 2)):
        s = mac_stokes(dim, n, 0.01)
        _, _, aux = auxiliary_space_preconditioner(s)
        assert len(set(id(c) for c in aux.components)) == 1 and len(aux.components) == dim
        assert len(aux.components[0].level_sizes) >= min_levels, aux.components[0].level_sizes
        x = hipla.Vector.from_numpy(np.random.default_rng(3).standard_normal(s.n_u))
        out = {}
        for on in (0, 1):
            with hip_engine.overrides(amg_batch=on):
                y = hipla.Vector(s.n_u)
                aux.Mult(x, y)
                z = hipla.Vector.from_numpy(np.ones(s.n_u))
                aux.MultAdd(0.5, x, z)
                out[on] = (y.numpy(), z.numpy())
        for a, b in zip(out[0], out[1]):
            assert np.linalg.norm(a - b) <= 1e-13 * np.linalg.norm(a)
        # ... and inside the fused loop (multiplicative MypreA: the term is applied to the residual between the sweeps)
        f, g = s.rhs(0)
        A, B = hipla.SparseMatrix.from_scipy(s.A), hipla.SparseMatrix.from_scipy(s.B)
        hist = {}
        for on in (0, 1):
            with hip_engine.overrides(amg_batch=on):
                preA = MypreA(None, Form(A), s.line_blocks(3), GS=True, aux=aux)
                sol = hipla.BlockVector([hipla.Vector(s.n_u), hipla.Vector(s.n_p)])
                with contextlib.redirect_stdout(io.StringIO()):
                    ses = BpcgSession(Form(A), Form(B), None, hipla.Vector.from_numpy(f), hipla.Vector.from_numpy(g), preA,
                                      hipla.DiagonalMatrix(1.0 / s.mass), sol=sol)
                assert ses.fused is not None
                ses.first_direction()
                ses.fused.start(ses.wdn, ses.err0, 0.0, True, 25)
                ses.fused.enqueue(0, 25)
                ses.fused.poll()
                hist[on] = ses.fused.history(24).copy()
        np.testing.assert_allclose(hist[1], hist[0], rtol=1e-9)
        assert hist[1][-1] < 1e-1 * hist[1][0]


def test_fused_cg_solver(hip_engine):
    """hipla.CGSolver on native operands takes the device-resident loop (nss_cg_*): same history as
    the protocol loop, all preconditioner kinds, config-1 CG against the golden."""
    import heat
    import hipla
    from hipla import fused
    s = mac_stokes(3, 9, 0.01)
    A = hipla.SparseMatrix.from_scipy(s.A)
    b = np.random.default_rng(1).standard_normal(s.n_u)
    bv = hipla.Vector.from_numpy(b)
    import scipy.sparse.linalg as spl
    exact = spl.spsolve(s.A.tocsc(), b)
    pres = {"none": None, "jacobi": hipla.JacobiPreconditioner(A), "bjac": hipla.BlockJacobi(A, s.line_blocks(3)),
            "bgs": hipla.BlockGaussSeidel(A, s.line_blocks(3)), "amg": hipla.SmoothedAggregationAMG(A, coarse_size=200)}
    for name, pre in pres.items():
        runs = {}
        for mode in ("fused", "protocol"):
            fused.ENABLED = mode == "fused"
            try:
                cg = hipla.CGSolver(A, pre=pre, precision=1e-10, maxsteps=2000)
                x = hipla.Vector(s.n_u)
                x.data = cg * bv
                assert (cg._fused is not None) == (mode == "fused")
                runs[mode] = (cg.iterations, np.array(cg.errors), x.numpy())
            finally:
                fused.ENABLED = True
        (it_f, e_f, x_f), (it_p, e_p, x_p) = runs["fused"], runs["protocol"]
        assert abs(it_f - it_p) <= max(2, int(0.03 * it_p)), (name, it_f, it_p)
        m = min(25, len(e_f), len(e_p))
        np.testing.assert_allclose(e_f[:m], e_p[:m], rtol=1e-8)
        assert np.linalg.norm(x_f - exact) < 1e-7 * np.linalg.norm(exact), name
    assert runs["fused"][0] < 60                                     # AMG-preconditioned CG
    d = np.load(golden_path("cfg1_heat_plumbing"))
    from staggered_grid import diffusion_2d
    M = hipla.SparseMatrix.from_scipy(diffusion_2d(int(d["n"])))
    rhs = hipla.Vector.from_numpy(np.random.default_rng(int(d["seed"])).standard_normal(M.height))
    x, errors = heat.conjugate_gradients_fused(M, rhs, tol=1e-10)
    assert len(errors) - 1 == int(d["cg_iterations"])
    np.testing.assert_allclose(errors, d["cg_history"], rtol=1e-8)


def test_multiplicative_mypre_a_over_blocks_with_uncovered_dofs(hip_engine):
    """BPCG v2 with the multiplicative MypreA (GS=True, templates/NavierStokesSIMPLE_iterative.py:376-381) over blocks
    that leave velocity dofs uncovered (line blocks without the ones at the west wall, as blocks of free dofs only
    are): after `y += aux r` the back sweep starts from an iterate that is non-zero at those dofs, and it must read
    their coupling to the blocks.  The fused loop runs; history, iteration count and solution against kr.bpcg_v2 with
    kr.mypre_a (sequential sweeps in the GPU's colour-major block order, the GPU's auxiliary term as a black box)."""
    import hipla
    from solvers.bramblepasciak_new import BpcgSession, BramblePasciakCG
    from templates.NavierStokesSIMPLE_iterative import MypreA, auxiliary_space_preconditioner
    s = mac_stokes(2, 16, 0.01)
    idx = s.line_blocks(3)
    west = np.concatenate([g[..., 0].ravel() for g in s.component_ids])
    blocks = np.ascontiguousarray(idx[:, ~np.isin(idx, west).any(axis=0)])
    f, g = s.rhs(0)
    A, B = hipla.SparseMatrix.from_scipy(s.A), hipla.SparseMatrix.from_scipy(s.B)
    _, _, aux = auxiliary_space_preconditioner(s)
    preA = MypreA(None, Form(A), blocks, GS=True, aux=aux)
    assert preA.n_uncovered > 0
    preS = hipla.DiagonalMatrix(1.0 / s.mass)
    fv, gv = hipla.Vector.from_numpy(f), hipla.Vector.from_numpy(g)
    tol, maxsteps = 1e-9, 2000

    def aux_apply(r):
        y = hipla.Vector(s.n_u)
        aux.Mult(hipla.Vector.from_numpy(r), y)
        return y.numpy()

    pa, ps = kr.mypre_a(s.A, preA.idx_host, aux_apply, gs=True), kr.diag_inverse(s.mass)
    with contextlib.redirect_stdout(io.StringIO()):
        ses = BpcgSession(Form(A), Form(B), None, fv, gv, preA, preS)
    assert ses.fused is not None
    k = kr.scale_factor(kr.lanczos_ritz(s.A, pa, tol=1e-3))
    assert abs(k - ses.k) < 1e-8 * k
    out = io.StringIO()
    sol = hipla.BlockVector([hipla.Vector(s.n_u), hipla.Vector(s.n_p)])
    with contextlib.redirect_stdout(out), fused_loops_counted() as counts:
        it, _ = BramblePasciakCG(Form(A), Form(B), None, fv, gv, preA, preS, sol, tol=tol, maxsteps=maxsteps)
    assert counts["bpcg2"] == 1, "the fused device loop did not run: %r" % (counts,)
    hist = np.array([float(m) for m in re.findall(r"it =\s+\d+\s+err =\s+(\S+)", out.getvalue())])
    it_ref, u_ref, p_ref, hist_ref, _ = kr.bpcg_v2(s.A, s.B, pa, ps, f, g, k, tol=tol, maxsteps=maxsteps)
    w = min(20, len(hist), len(hist_ref))
    np.testing.assert_allclose(hist[:w], hist_ref[:w], rtol=1e-8)
    # the band of the other MypreA solver test (test_auxiliary_space_mypre_a_native_in_the_fused_loop): the oracle's
    # sweeps solve the blocks with LAPACK, the GPU with packed inverses -- ~300 iterations drift by a few percent
    assert abs(it - it_ref) <= max(3, int(0.05 * it_ref))
    x_ref = np.concatenate([u_ref, p_ref])
    assert np.linalg.norm(sol.numpy() - x_ref) < 1e-5 * np.linalg.norm(x_ref)
    # (no bound on the saddle-point residual here: the uncovered dofs are reached by the auxiliary term only, and the
    # stop test on the preconditioned functional fires with a true residual of ~10 % -- on the oracle's side as well,
    # which is what this test pins)
    b, K = np.concatenate([f, g]), s.saddle_matrix()
    r, r_ref = np.linalg.norm(b - K @ sol.numpy()), np.linalg.norm(b - K @ x_ref)
    assert abs(r - r_ref) < 1e-3 * r_ref + 1e-6 * np.linalg.norm(b)
    assert 3 < it < 400
