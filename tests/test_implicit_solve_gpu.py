"""`hipla.stepping.ImplicitSolve` on its own, on the product engine: both quantities (the velocity's M_u, A, [A | D] and
the scalar's M_p, K, [K | B]) and every kind on the smallest grids of tests/test_implicit_convection_gpu.py, each solve
against `spsolve` of the assembled M + theta tau L -- for "bicgstab" of M + tau (L + N(a)), assembled as
`LinearisedConvection.to_scipy` assembles it -- and the parts a kind does not use against None.  The kinds that take the
step size per solve run two sizes in succession through one object.

Bounds, those of the existing comparisons.  The CG kinds: solves at precision 1e-14 agree to 1e-10, the bound of
`test_shifted_solves` (tests/test_variable_step_gpu.py); the direct solve, which has no precision, is held to the same.
"bicgstab": solves at 1e-12 agree with `spsolve` to 1e-9, the bound of `test_form_two_on_grids_against_spsolve`."""

import functools

import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spl

from oracle import krylov_ref as kr

pytestmark = pytest.mark.gpu

TAUS = (0.05, 0.0125)
WALLS = {"x-": 1.0, "x+": 0.0}
PARTS = ("assembled", "pre", "cg", "fdm", "bicg", "dinv", "a")
CASES = {   # case -> (kind, inner_pre, with the direct inverse, the parts it holds)
    "cg jacobi": ("cg", "jacobi", False, {"assembled", "pre", "cg"}),
    "cg amg": ("cg", "amg", False, {"assembled", "pre", "cg"}),
    "shifted": ("shifted", "jacobi", False, {"cg"}),
    "fdm": ("fdm", "amg", True, {"fdm"}),
    "bicgstab jacobi": ("bicgstab", "jacobi", False, {"bicg", "dinv", "a"}),
    "bicgstab fdm": ("bicgstab", "amg", True, {"bicg", "fdm", "a"}),
}


def rel(a, b):
    return np.linalg.norm(np.asarray(a) - b) / np.linalg.norm(b)


@functools.lru_cache(maxsize=None)
def quantity(which, dim, n):
    """The host operands of one quantity on the grid: mass, L, the rows [L | Dv], avg, diff, the advecting field a (at
    tau * CflRate = 4 for the larger step, as in `test_form_two_on_grids_against_spsolve`), the index arrays of the
    fast diagonalisation, the keys of `shared` and a right-hand side."""
    from staggered_grid import mac_stokes
    s = mac_stokes(dim, n, 0.01)
    m_u = np.full(s.n_u, s.h ** s.dim)
    u = kr.project(s.B, m_u, np.random.default_rng(2).standard_normal(s.n_u))[0]
    u *= 4.0 / (TAUS[0] * ((abs(s.B) @ np.abs(u)) / s.mass).max())
    if which == "velocity":
        ops = s.convection_operators()
        q = dict(mass=m_u, lap=s.A.tocsr(), div=ops["div"], avg=ops["avg"], diff=ops["diff"], a=ops["adv"] @ u,
                 ids=s.component_ids, keys=dict(assembled="mstar", diag="diagA"), label="the velocity solve")
    else:
        ops = s.scalar_operators(0.8, WALLS)
        q = dict(mass=ops["mass"], lap=sp.csr_matrix(ops["K"]), div=s.B, avg=ops["avg"], diff=ops["diff"], a=u,
                 ids=[np.arange(s.n_p).reshape((n,) * dim)], keys=dict(assembled="mstar", lap="K", diag="diagK"),
                 label="the scalar's solve")
    rows = sp.hstack([q["lap"], q["div"]], format="csr")
    rows.sort_indices()
    conv = q["div"] @ (sp.diags(q["a"]) @ q["avg"] - sp.diags(0.5 * np.abs(q["a"])) @ q["diff"])
    q.update(rows=rows, conv=conv, rhs=np.random.default_rng(1).standard_normal(q["lap"].shape[0]))
    return q


@pytest.mark.parametrize("case", list(CASES))
@pytest.mark.parametrize("dim,n", [(2, 5), (3, 3)])
@pytest.mark.parametrize("which", ["velocity", "scalar"])
def test_every_kind_against_spsolve(hip_engine, which, dim, n, case):
    import hipla
    from hipla.stepping import ImplicitSolve
    eng = hip_engine
    kind, inner_pre, direct, held = CASES[case]
    q = quantity(which, dim, n)
    size = q["lap"].shape[0]
    # the velocity hands over the matrix it holds, the scalar its host K
    lap = hipla.SparseMatrix.from_scipy(q["lap"]) if which == "velocity" else q["lap"]
    rows, avg, diff = (hipla.SparseMatrix.from_scipy(q[key]) for key in ("rows", "avg", "diff"))
    rhs, out = eng.from_host(q["rhs"]), eng.zeros(size)
    for theta in (1.0, 0.5) if kind != "bicgstab" else (1.0,):       # ("bicgstab" is an "euler" stepper's)
        shared = {}
        inverse = hipla.ComponentFastDiagonalization.try_create(q["lap"], q["ids"], q["mass"], TAUS[0]) if direct else None
        assert not direct or (inverse is not None and inverse.handle is not None)
        solve = ImplicitSolve(eng, kind, q["label"], inner_pre, TAUS[0], theta, q["mass"], lap, shared, q["keys"], inverse,
                              rows, avg, diff)
        assert solve.kind == kind and {name for name in PARTS if getattr(solve, name) is not None} == held
        assert solve.fdm is inverse and (solve.assembled is None or solve.assembled is shared["mstar"])
        assert set(shared) == {"cg": {"mstar"}, "shifted": set(q["keys"].values()) - {"mstar"}}.get(kind, set())
        if kind == "shifted":                   # the loop runs on the caller's own matrix, or on the uploaded "K"
            assert solve.cg.mat is (lap if which == "velocity" else shared["K"])
        if kind == "bicgstab":
            assert solve.bicg.mat is rows and solve.a.numel() == len(q["a"])
            eng.upload(q["a"], solve.a)
        precision, maxsteps, bound = (1e-12, 2000, 1e-9) if kind == "bicgstab" else (1e-14, 5000, 1e-10)
        for step, tau in enumerate(TAUS[:1] if kind == "cg" else TAUS):
            its = solve.solve(rhs, out, tau, precision, maxsteps, step)
            full = sp.diags(q["mass"]) + theta * tau * (q["lap"] + q["conv"] if kind == "bicgstab" else q["lap"])
            err = rel(eng.to_host(out), spl.spsolve(full.tocsc(), q["rhs"]))
            print("%s %d-D n = %d, %s, theta %g, tau %g: %d iterations, %.3g from spsolve"
                  % (which, dim, n, case, theta, tau, its, err))
            assert (its == 0 if kind == "fdm" else 0 < its < maxsteps) and err <= bound
            if kind == "shifted":
                assert solve.cg.sigma == theta * tau
