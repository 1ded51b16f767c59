"""Shared by tests/golden/make_stabilised_golden.py and the tests of the stabilised saddle-point systems
``[[A, B^T], [B, C]]``: turns the inputs recorded in a ``stab_*.npz`` fixture back into the assembled system with its
lower-right block, runs the two entry points that take one, and checks a solution against the matrix WITH C
(`check_solution` of test_hip_solvers.py uses ``saddle_matrix()``, which has none).  Host-only numpy/scipy apart from
`device_operands` / `run_entry_point`, which go through whatever engine is installed.

Fixture inputs: ``dim, n, nu, seed, pre`` as golden_cases.Case, ``eps`` (C = pressure_stabilisation(eps)); the
right-hand side is f = rhs(seed)[0] and g = default_rng(1).standard_normal(n_p) minus its mean (a g in the range of
the singular system: C annihilates the constants as B^T does)."""

import contextlib
import io
import os
import re

import numpy as np
import scipy.sparse as sp

from golden_cases import Case

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

# (dim, n, eps, pre): the block-Jacobi case runs the epilogue of A's rows planned around the blocks (plan_for_blocks)
GRID = [(2, 3, 0.5, "jacobi"), (2, 12, 1.0, "jacobi"), (3, 6, 1.0, "jacobi"), (2, 12, 1.0, "bjac")]
SOLVERS = ("bpcg1", "minres")
TOL, MAXSTEPS, NU, G_SEED = 1e-8, 3000, 0.01, 1


def tag(dim, n, pre, solver):
    return "stab_%dd_n%d_%s_%s" % (dim, n, pre, solver)


NAMES = [tag(dim, n, pre, solver) for dim, n, _, pre in GRID for solver in SOLVERS]


def load(name):
    return np.load(os.path.join(GOLDEN, name + ".npz"))


class StabCase(Case):
    """A golden_cases.Case with the stabilisation block: `C` (scipy CSR), `eps`, and g as described above."""

    def __init__(self, d):
        super().__init__(d)
        self.eps = float(d["eps"])
        self.C = self.system.pressure_stabilisation(self.eps)
        g = np.random.default_rng(G_SEED).standard_normal(self.system.n_p)
        self.g = g - g.mean()

    def matrix(self):
        s = self.system
        return sp.bmat([[s.A, s.B.T], [s.B, self.C]], format="csr")


def params(dim, n, eps, pre):
    return dict(dim=dim, n=n, nu=NU, seed=0, pre=pre, inflate=1, condense=0, eps=eps)


def check_solution(x, case, d):
    """The true residual with the matrix that holds C, the norm and the samples: the bounds of test_hip_solvers.py."""
    b = case.rhs
    res = np.linalg.norm(b - case.matrix() @ x)
    assert res <= 10 * max(float(d["residual"]), 1e-12 * float(d["b_norm"])), (res, float(d["residual"]))
    assert abs(np.linalg.norm(x) - float(d["x_norm"])) <= 1e-6 * float(d["x_norm"])
    np.testing.assert_allclose(x[d["sample_idx"]], d["sample_val"], rtol=0, atol=1e-6 * np.abs(x).max())


def check_history(h, ref, window, rtol=1e-8):
    w = min(int(window), len(h), len(ref))
    rel = np.abs(np.asarray(h[:w]) - ref[:w]) / np.abs(ref[:w])
    assert rel.max() <= rtol, rel.max()


def device_operands(case, C=True):
    """(A, B, C, preA, preS) on the installed engine; `C`: True = the case's, None, or a scipy matrix."""
    import hipla
    s = case.system
    A, B = hipla.SparseMatrix.from_scipy(s.A), hipla.SparseMatrix.from_scipy(s.B)
    Cs = case.C if C is True else C
    Cm = None if Cs is None else hipla.SparseMatrix.from_scipy(sp.csr_matrix(Cs))
    preA = hipla.DiagonalMatrix(case.jacobi_diagonal()) if case.blocks is None else hipla.BlockJacobi(A, case.blocks)
    return A, B, Cm, preA, hipla.DiagonalMatrix(1.0 / s.mass)


def solve(solver, case, ops, tol=TOL, maxsteps=MAXSTEPS, warm=None):
    """One run of `solver`'s entry point.  Returns (x, errors, printed text, returned vector is `warm`'s)."""
    import hipla
    from bramble_pasciak_cg import bramble_pasciak_cg
    from minres import MinRes
    A, B, Cm, preA, preS = ops
    fv, gv = hipla.Vector.from_numpy(case.f), hipla.Vector.from_numpy(case.g)
    start = None
    if warm is not None:
        start = hipla.BlockVector([hipla.Vector.from_numpy(warm[0]), hipla.Vector.from_numpy(warm[1])])
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        if solver == "bpcg1":
            kw = {} if start is None else {"solution": start}
            sol, errors = bramble_pasciak_cg(A, B, Cm, preA, preS, fv, gv, tolerance=tol, max_steps=maxsteps,
                                             print_rates=False, **kw)
        else:
            K = hipla.BlockMatrix([[A, B.T], [B, Cm]])
            P = hipla.BlockMatrix([[preA, None], [None, preS]])
            kw = {} if start is None else {"sol": start, "initialize": False}
            sol, errors = MinRes(mat=K, pre=P, rhs=hipla.BlockVector([fv, gv]), maxsteps=maxsteps, tol=tol,
                                 printrates=False, **kw)
    return sol.numpy(), np.asarray(errors), out.getvalue(), start is not None and sol is start


def run_entry_point(d, case, ops):
    """The entry point of fixture `d` against it: history to 1e-8 over the stable window, the iteration count inside
    `band` (conftest.iteration_tolerance), k, the warning and the solution."""
    from conftest import iteration_tolerance
    solver = str(d["solver"])
    x, errors, text, _ = solve(solver, case, ops, float(d["tol"]), int(d["maxsteps"]))
    if solver == "bpcg1":
        k = float(re.search(r"scale factor:\s+(\S+)", text).group(1))
        assert abs(k - float(d["k"])) <= 1e-8 * k
    check_history(errors, d["errors"], d["window"])
    band = iteration_tolerance(d)
    assert abs(len(errors) - 1 - int(d["iterations"])) <= band, (len(errors) - 1, int(d["iterations"]), band)
    assert ("Warning" in text) == bool(d["warned"])
    check_solution(x, case, d)
    return x, errors
