#!/usr/bin/env python3
"""Generate tests/golden/stab_*.npz: the reference's *unmodified* ``bramble_pasciak_cg`` and ``MinRes`` on stabilised
saddle-point systems ``[[A, B^T], [B, C]]`` with C = StokesSystem.pressure_stabilisation(eps).

As make_golden.py (whose backends, `stable_window` and `_ReversedDot` this file imports and does not touch): the
reference's files run over ``tests/ngsolve_numpy`` -- these runs are what the fixtures store -- and once more over the
product's protocol layer on the numpy checker engine, which must agree (`cross_check`: make_golden.py's bounds,
except that the iteration counts may differ by conftest.iteration_tolerance, the band the tests hold the product to
-- the two stand-ins differ by 3 iterations in 260 on the 2-D n = 12 system, with equal histories over the window).
The stable window and ``iterations_perturbed`` come from a second reference run with the summation order of every
inner product reversed (oracle/krylov_ref.py::bpcg_v1 has no C, so the reference is perturbed itself).  Every case
must converge without the reference's warning, or this script fails.

Nothing of the reference is written to the repo: only inputs (generator parameters, seeds, eps) and outputs.

    python tests/golden/make_stabilised_golden.py <reference checkout>     # rewrites tests/golden/stab_*.npz
"""

import contextlib
import io
import os
import sys

import numpy as np

import make_golden as mg                         # (puts the repository, the package and tests/ on sys.path)
from make_golden import HEAD, HiplaBackend, NumpyBackend, _ReversedDot, samples, stable_window

import stabilised_cases as sc                    # noqa: E402
from conftest import iteration_tolerance         # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))


def run_v1(be, case):
    s = case.system
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        sol, errors = be.v1.bramble_pasciak_cg(be.sparse(s.A), be.sparse(s.B), be.sparse(case.C), be.preA(case),
                                               be.diag(1.0 / s.mass), be.vec(case.f), be.vec(case.g),
                                               tolerance=sc.TOL, max_steps=sc.MAXSTEPS, print_rates=False)
    return dict(x=be.numpy(sol), hist=np.array(errors), lams=be.lams.copy(), warned="Warning" in out.getvalue())


def run_minres(be, case):
    s = case.system
    A, B = be.sparse(s.A), be.sparse(s.B)
    K = be.block_matrix([[A, B.T], [B, be.sparse(case.C)]])
    P = be.block_matrix([[be.preA(case), None], [None, be.diag(1.0 / s.mass)]])
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        u, errs = be.minres.MinRes(mat=K, pre=P, rhs=be.block([be.vec(case.f), be.vec(case.g)]),
                                   maxsteps=sc.MAXSTEPS, tol=sc.TOL, printrates=False)
    return dict(x=be.numpy(u), hist=np.array(errs), warned="Warning" in out.getvalue())


def cross_check(name, a, b, window, band):
    """Outputs of the two stand-ins: `a` (numpy-only, stored) against `b` (the product's protocol layer)."""
    if "lams" in a:
        rel = abs(a["lams"].min() - b["lams"].min()) / abs(a["lams"].min())
        assert rel <= 1e-12, (name, "lam_min", rel)
    m = min(len(a["hist"]), len(b["hist"]))
    rel = np.abs(a["hist"][:m] - b["hist"][:m]) / np.abs(a["hist"][:m])
    head, inwin = float(rel[:HEAD].max()), float(rel[: min(m, window)].max())
    assert head <= 1e-12, (name, "history head", head)
    assert inwin <= 1e-9, (name, "history window", inwin)
    assert abs(len(a["hist"]) - len(b["hist"])) <= band, (name, len(a["hist"]), len(b["hist"]), band)
    denom = np.linalg.norm(a["x"])
    assert np.linalg.norm(a["x"] - b["x"]) <= 1e-7 * denom, (name, "solution", np.linalg.norm(a["x"] - b["x"]) / denom)
    assert a["warned"] == b["warned"], (name, "warned")
    return {"standin_head_rel_diff": head, "standin_window_rel_diff": inwin,
            "standin_iteration_diff": len(b["hist"]) - len(a["hist"])}


def main():
    numpy_be, hipla_be = NumpyBackend(), HiplaBackend()
    for dim, n, eps, pre in sc.GRID:
        params = sc.params(dim, n, eps, pre)
        case = sc.StabCase(params)
        s = case.system
        K, b = case.matrix(), case.rhs
        common = dict(n_u=s.n_u, n_p=s.n_p, **params)
        for solver, run in (("bpcg1", run_v1), ("minres", run_minres)):
            name = sc.tag(dim, n, pre, solver)
            r = run(numpy_be, case)
            with _ReversedDot():
                rp = run(numpy_be, case)
            r2 = run(hipla_be, case)
            assert not r["warned"] and not rp["warned"], (name, "the reference did not converge")
            its, itp = len(r["hist"]) - 1, len(rp["hist"]) - 1
            assert its < sc.MAXSTEPS and r["hist"][-1] < sc.TOL, (name, its, r["hist"][-1])
            W = stable_window(r["hist"], rp["hist"])
            rep = cross_check(name, r, r2, W, iteration_tolerance(dict(iterations=its, iterations_perturbed=itp)))
            si, sv = samples(r["x"])
            extra = {}
            if solver == "bpcg1":
                extra = dict(k=1.0 / r["lams"].min() + 1e-3, lam_min=r["lams"].min(), lam_max=r["lams"].max())
            path = os.path.join(HERE, name + ".npz")
            np.savez_compressed(path, solver=solver, tol=sc.TOL, maxsteps=sc.MAXSTEPS, errors=r["hist"], iterations=its,
                                iterations_perturbed=itp, window=W, x_norm=np.linalg.norm(r["x"]),
                                residual=np.linalg.norm(b - K @ r["x"]), b_norm=np.linalg.norm(b), sample_idx=si,
                                sample_val=sv, warned=r["warned"], **extra, **rep, **common)
            print("%-32s %6d B  iterations %4d (perturbed %4d)  window %3d  stand-ins differ by %.1e inside it"
                  % (name, os.path.getsize(path), its, itp, W, rep["standin_window_rel_diff"]))


if __name__ == "__main__":
    if len(sys.argv) != 2 or not os.path.isdir(sys.argv[1]):
        raise SystemExit("usage: make_stabilised_golden.py <checkout of matschiner/navier-stokes-solver>")
    mg.REF = os.path.abspath(sys.argv[1])
    main()
