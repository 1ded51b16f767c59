"""Linearly implicit convection on the CPU checker engine: the host restatements, `LinearisedConvection` and
`BiCGStabSolver` through the protocol, `DoTimeStep` / `Advance` after `SetConvectionTreatment("implicit")` against the
numpy reference step (tests/implicit_convection_reference.py), the refusals, the unchanged default, and the energy
bound of the scheme.

Bounds.  Restatements: 1e-14 of max |conv| (measured 1.6e-16: the same products in another order).  Solves run at a
relative residual of 1e-12 on operators of condition number below 1e3, so iterates agree with `spsolve` to 1e-9, the
project's bound for such twins (tests/test_implicit_fdm_gpu.py)."""

import contextlib
import io

import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spl

import implicit_convection_reference as icr
from oracle import krylov_ref as kr

WALLS = {"x-": 1.0, "x+": 0.0}
GRIDS = {"2d": (2, 6, (0.0, 2.0)), "3d": (3, 4, (0.0, 2.0, -1.0))}
TAU = 0.05
TIGHT = dict(precision=(1e-12, 1e-13), maxsteps=(4000, 20000))


def rel(a, b):
    return np.linalg.norm(np.asarray(a) - b) / np.linalg.norm(b)


def quiet(call, *args, **kw):
    with contextlib.redirect_stdout(io.StringIO()):
        return call(*args, **kw)


def fresh(grid, buoyant=False, treatment=None, implicit=None, **kw):
    import hipla
    from templates.NavierStokesSIMPLE_iterative import NavierStokes, SyntheticMesh
    dim, n, beta = GRIDS[grid] if isinstance(grid, str) else grid
    ns = NavierStokes(SyntheticMesh(1.0 / n, dim=dim), nu=0.01, inflow="inlet", outflow="outlet", wall="wall|cyl",
                      uin=None, timestep=TAU, order=0, **kw)
    s = ns.system
    ns.f.vec.data = hipla.Vector.from_numpy(0.5 * s.h ** s.dim * np.random.default_rng(8).standard_normal(s.n_u))
    u0 = 0.2 * kr.project(s.B, np.full(s.n_u, s.h ** s.dim), np.random.default_rng(2).standard_normal(s.n_u))[0]
    ns.gfu.data = hipla.Vector.from_numpy(u0)
    if buoyant:
        ns.AddScalar(initial=np.random.default_rng(6).random(s.n_p), precision=1e-14, maxsteps=5000, kappa=0.8,
                     dirichlet=WALLS, buoyancy=beta, t_ref=0.5)
    if implicit is not None:
        ns.SetImplicitSolve(implicit)
    if treatment is not None:
        ns.SetConvectionTreatment(treatment)
    return ns


def tighten(ns):
    """The statement path's solvers at 1e-12 (velocity) and 1e-13 (projection); the scalar's comes from `AddScalar`."""
    ops = ns._time_stepping_operators()
    ops["invproj"].precision, ops["invproj"].maxsteps = 1e-13, 20000
    ops["invmstar"].precision, ops["invmstar"].maxsteps = 1e-12, 5000
    if ns.convection_treatment == "implicit":
        inv = ns._implicit_momentum_solver(None)
        inv.precision, inv.maxsteps = 1e-12, 4000


def scalar_of(ns):
    sc = ns._scalar
    return None if sc is None else dict(ops=sc.ops, T=ns.temperature.numpy().copy(), w_b=sc.w_b, t_ref=sc.t_ref)


def assert_state(ns, ref, what):
    errs = [rel(ns.gfu.numpy(), ref["u"])]
    p, q = ns.gfup.numpy(), ref["phi"]
    errs.append(rel(p - p.mean(), q - q.mean()))
    if "T" in ref:
        errs.append(rel(ns.temperature.numpy(), ref["T"]))
    print("%s: relative differences (u, gfup, T) %s" % (what, ["%.3g" % e for e in errs]))
    assert max(errs) <= 1e-9, errs


# ---- operator and restatement ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim,n", [(2, 6), (2, 8), (3, 4)])
def test_restatement_reproduces_the_explicit_term(dim, n):
    from staggered_grid import mac_stokes
    s = mac_stokes(dim, n, 0.01)
    ops = s.convection_operators()
    rng = np.random.default_rng(dim * 10 + n)
    u, v, w = (rng.standard_normal(s.n_u) for _ in range(3))
    conv = s.convection_reference(u)
    N = s.linearised_convection(ops["adv"] @ u)
    err = abs(N @ u + conv).max() / abs(conv).max()
    print("N(I_adv u) u + conv(u): %.3g of max |conv|" % err)
    assert err <= 1e-14
    assert N.shape == (s.n_u, s.n_u) and abs(N - N.T).max() > 0.0              # nonsymmetric
    a = rng.standard_normal(ops["avg"].shape[0])
    a[::5] = 0.0
    Na = s.linearised_convection(a, ops)
    flux = a * (ops["avg"] @ v) - 0.5 * np.abs(a) * (ops["diff"] @ v)
    assert abs(Na @ v - ops["div"] @ flux).max() <= 1e-14 * abs(ops["div"] @ flux).max()
    lin = Na @ (2.0 * v - 3.0 * w) - (2.0 * (Na @ v) - 3.0 * (Na @ w))
    assert abs(lin).max() <= 1e-13 * abs(Na @ v).max()                          # linear in v
    with pytest.raises(ValueError):
        s.linearised_convection(a[:-1])


@pytest.mark.parametrize("dim,n", [(2, 6), (3, 4)])
def test_scalar_restatement(dim, n):
    from staggered_grid import mac_stokes
    s = mac_stokes(dim, n, 0.01)
    sops = s.scalar_operators(0.8, WALLS)
    rng = np.random.default_rng(3)
    u, T = rng.standard_normal(s.n_u), rng.standard_normal(s.n_p)
    ref = s.scalar_convection_reference(u, T).ravel()
    err = abs(s.linearised_scalar_convection(u, sops) @ T + ref).max() / abs(ref).max()
    print("B G(u; T) + scalar_convection_reference: %.3g" % err)
    assert err <= 1e-14


@pytest.mark.parametrize("dim,n", [(2, 6), (3, 4)])
@pytest.mark.parametrize("uniform", [True, False])
def test_linearised_convection_operator_against_the_restatement(numpy_engine, dim, n, uniform):
    import hipla
    from hipla.stepping import LinearisedConvection
    from staggered_grid import mac_stokes
    s = mac_stokes(dim, n, 0.01)
    ops = s.convection_operators()
    rng = np.random.default_rng(5)
    mass = np.full(s.n_u, s.h ** s.dim) if uniform else s.h ** s.dim * (0.5 + rng.random(s.n_u))
    op = LinearisedConvection(ops, mass, s.A, sigma=0.3)
    u, x = rng.standard_normal(s.n_u), rng.standard_normal(s.n_u)
    with pytest.raises(ValueError):
        op.Mult(hipla.Vector.from_numpy(x), hipla.Vector(s.n_u))                # not frozen yet
    op.freeze(hipla.Vector.from_numpy(u))
    for sigma in (0.3, 0.0, 2.5):
        op.sigma = sigma
        M = sp.diags(mass) + sigma * (s.A + s.linearised_convection(ops["adv"] @ u, ops))
        y = hipla.Vector(s.n_u)
        y.data = op * hipla.Vector.from_numpy(x)
        assert abs(y.numpy() - M @ x).max() <= 1e-13 * abs(M @ x).max()
        assert abs(op.to_scipy() - M).max() <= 1e-15 * abs(M).max()
        assert np.allclose(numpy_engine.to_host(op.jacobi().d), 1.0 / M.diagonal(), rtol=1e-14, atol=0.0)
    sops = s.scalar_operators(0.8, WALLS)                                       # the scalar twin: a = the face velocities
    ops_T = dict(avg=sops["avg"], diff=sops["diff"], div=s.B)
    op_T = LinearisedConvection(ops_T, sops["mass"], sops["K"], sigma=0.7)
    op_T.freeze(hipla.Vector.from_numpy(u))
    T = rng.standard_normal(s.n_p)
    M = sp.diags(sops["mass"]) + 0.7 * (sops["K"] + s.linearised_scalar_convection(u, sops))
    y = hipla.Vector(s.n_p)
    y.data = op_T * hipla.Vector.from_numpy(T)
    assert abs(y.numpy() - M @ T).max() <= 1e-13 * abs(M @ T).max()
    with pytest.raises(ValueError):
        op.sigma = -1.0


# ---- the solver through the protocol -----------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 63, 257])
@pytest.mark.parametrize("jacobi", [False, True])
def test_bicgstab_solver_through_the_protocol(numpy_engine, n, jacobi):
    import hipla
    A = icr.nearly_identity(n, seed=n)
    b = np.random.default_rng(n + 1).standard_normal(n)
    mat = hipla.SparseMatrix.from_scipy(A)
    pre = hipla.DiagonalMatrix(1.0 / A.diagonal()) if jacobi else None
    inv = hipla.BiCGStabSolver(mat, pre, precision=1e-12, maxsteps=200)
    x = hipla.Vector(n)
    x.data = inv * hipla.Vector.from_numpy(b)
    ref = spl.spsolve(A.tocsc(), b) if n > 1 else b / A.toarray()[0, 0]
    assert rel(x.numpy(), ref) <= 1e-9
    its, hist, code = icr.bicgstab(A, b, (lambda v: v / A.diagonal()) if jacobi else None, 1e-12, 200)
    assert code == 0 and inv.iterations == len(hist) and len(inv.errors) == inv.iterations + 1
    assert np.allclose(inv.errors[1:], hist, rtol=1e-6, atol=1e-14 * inv.errors[0])
    assert inv.errors[0] == pytest.approx(np.linalg.norm(b), rel=1e-14)


def test_bicgstab_solver_edges(numpy_engine):
    import hipla
    eye = hipla.SparseMatrix.from_scipy(sp.identity(5, format="csr"))
    inv = hipla.BiCGStabSolver(eye, precision=1e-10)
    b = np.array([1.0, -2.0, 3.0, 0.0, 4.0])
    x = hipla.Vector(5)
    x.data = inv * hipla.Vector.from_numpy(b)
    assert inv.iterations == 1 and np.array_equal(x.numpy(), b)                 # <t, t> == 0 is convergence here
    x.data = inv * hipla.Vector.from_numpy(np.zeros(5))
    assert inv.iterations == 0 and inv.errors == [0.0] and np.array_equal(x.numpy(), np.zeros(5))
    skew = hipla.SparseMatrix.from_scipy(sp.csr_matrix(np.array([[0.0, 1.0], [-1.0, 0.0]])))
    inv = hipla.BiCGStabSolver(skew)
    x = hipla.Vector(2)
    with pytest.raises(FloatingPointError, match="code 1"):
        x.data = inv * hipla.Vector.from_numpy(np.array([1.0, 0.0]))
    capped = hipla.BiCGStabSolver(hipla.SparseMatrix.from_scipy(icr.nearly_identity(65, 1)), precision=1e-30, maxsteps=3)
    y = hipla.Vector(65)
    y.data = capped * hipla.Vector.from_numpy(np.ones(65))
    assert capped.iterations == 3


@pytest.mark.parametrize("grid", ["2d", "3d"])
@pytest.mark.parametrize("pre", ["none", "jacobi", "fdm"])
def test_solver_on_the_grid_operator(numpy_engine, grid, pre):
    import hipla
    ns = fresh(grid, implicit="fdm" if pre == "fdm" else None)
    s = ns.system
    from hipla.stepping import LinearisedConvection
    m_u = np.full(s.n_u, s.h ** s.dim)
    op = LinearisedConvection(s.convection_operators(), m_u, s.A, sigma=0.0)
    u = ns.gfu.numpy()
    rate = ns.CflRate()
    op.freeze(hipla.Vector.from_numpy(u * (4.0 / (TAU * rate))))                # tau * CflRate = 4
    op.sigma = TAU
    P = None if pre == "none" else op.jacobi() if pre == "jacobi" else ns._fdm_u
    if pre == "fdm":
        P.sigma = TAU
    inv = hipla.BiCGStabSolver(op, P, precision=1e-12, maxsteps=2000)
    b = np.random.default_rng(1).standard_normal(s.n_u)
    x = hipla.Vector(s.n_u)
    x.data = inv * hipla.Vector.from_numpy(b)
    ref = spl.spsolve(op.to_scipy().tocsc(), b)
    print("%s %s: %d iterations, %.3g from spsolve" % (grid, pre, inv.iterations, rel(x.numpy(), ref)))
    assert rel(x.numpy(), ref) <= 1e-9


# ---- the step -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("grid", ["2d", "3d"])
@pytest.mark.parametrize("buoyant", [False, True])
@pytest.mark.parametrize("implicit", ["cg", "fdm"])
def test_do_time_step_against_the_reference_step(numpy_engine, grid, buoyant, implicit):
    ns = fresh(grid, buoyant, "implicit", implicit)
    assert ns.convection_treatment == "implicit"
    tighten(ns)
    s, f = ns.system, ns.f.vec.numpy().copy()
    u, sc = ns.gfu.numpy().copy(), scalar_of(ns)
    ref, _ = icr.reference_run(s, u, f, [TAU, 0.13, TAU], sc)
    quiet(ns.DoTimeStep)
    quiet(ns.DoTimeStep, timestep=0.13)                                          # a step of another size
    quiet(ns.DoTimeStep)
    assert ns._last_momentum_solver.iterations > 0
    assert_state(ns, ref, "%s buoyant=%s %s" % (grid, buoyant, implicit))


@pytest.mark.parametrize("mode", ["fixed", "timesteps", "cfl"])
def test_advance_by_statements_against_the_reference(numpy_engine, mode):
    ns = fresh("2d", True, "implicit")
    s, f, u, sc = ns.system, ns.f.vec.numpy().copy(), ns.gfu.numpy().copy(), scalar_of(ns)
    kw = {"fixed": {}, "timesteps": dict(timesteps=[0.05, 0.2, 0.1]), "cfl": dict(cfl=4.0, max_timestep=10.0)}[mode]
    rec = ns.Advance(3, **kw, **TIGHT)
    assert rec.declined is not None and rec.convection_treatment == "implicit"
    assert (rec.mstar_iterations > 0).all() and (rec.scalar_iterations > 0).all()
    taus = [TAU] * 3 if mode == "fixed" else list(rec.timestep)
    ref, energy = icr.reference_run(s, u, f, taus, sc)
    assert_state(ns, ref, "Advance by statements, " + mode)
    assert np.allclose(rec.kinetic_energy, energy, rtol=1e-9, atol=0.0)


def test_refusals(numpy_engine):
    from templates.NavierStokesSIMPLE_iterative import NavierStokes, SyntheticMesh
    with pytest.raises(ValueError, match="cnab2"):
        fresh("2d", time_scheme="cnab2").SetConvectionTreatment("implicit")
    with pytest.raises(ValueError, match="upwind"):
        fresh("2d", convection="minmod").SetConvectionTreatment("implicit")
    inflated = NavierStokes(SyntheticMesh(0.25, dim=2), nu=0.01, inflow="inlet", outflow="outlet", wall="wall|cyl",
                            uin=None, timestep=TAU, order=1)
    assert inflated.system.block_size > 1
    with pytest.raises(ValueError, match="block_size"):
        inflated.SetConvectionTreatment("implicit")
    replaced = fresh("2d")
    replaced.conv_operator = replaced.conv_operator
    with pytest.raises(ValueError, match="conv_operator"):
        replaced.SetConvectionTreatment("implicit")
    with pytest.raises(ValueError, match="explicit"):
        fresh("2d").SetConvectionTreatment("semi")
    ns = fresh("2d", treatment="implicit")
    with pytest.raises(ValueError, match="pseudo"):
        ns.Advance(1, pseudo=True)
    with pytest.raises(ValueError, match="amg"):
        ns.Advance(1, inner_pre="amg")
    ns.conv_operator = ns.conv_operator                                         # replaced after the switch
    with pytest.raises(ValueError, match="conv_operator"):
        quiet(ns.DoTimeStep)
    limited = fresh("2d", treatment="implicit")
    limited.AddScalar(kappa=0.8, dirichlet=WALLS, convection="vanleer")          # a limited scalar after the switch
    with pytest.raises(ValueError, match="upwind"):
        limited.Advance(1)
    for bad in (ns, limited):
        assert bad.convection_treatment == "implicit"


@pytest.mark.parametrize("buoyant", [False, True])
def test_switching_there_and_back_restores_the_bits(numpy_engine, buoyant):
    def run(switch):
        ns = fresh("2d", buoyant)
        if switch:
            ns.SetConvectionTreatment("implicit")
            quiet(ns.DoTimeStep)                                                 # an implicit step in between ...
            ns.SetConvectionTreatment("explicit")
            twin = fresh("2d", buoyant)                                          # ... and the start put back
            ns.gfu.data, ns.gfup.data = twin.gfu, twin.gfup
            if buoyant:
                ns.temperature.data = twin.temperature
            ns._clock.tau_prev = None
        assert ns.convection_treatment == "explicit"
        quiet(ns.DoTimeStep)
        quiet(ns.DoTimeStep, 0.03)
        recs = [ns.Advance(2), ns.Advance(2, timesteps=[0.02, 0.04])]
        assert all(r.convection_treatment == "explicit" for r in recs)
        out = [ns.gfu.numpy(), ns.gfup.numpy()] + ([ns.temperature.numpy()] if buoyant else [])
        return out + [r.mstar_iterations for r in recs] + [r.kinetic_energy for r in recs]
    for a, b in zip(run(False), run(True)):
        assert np.array_equal(a, b)


# ---- energy -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("grid,steps", [((2, 8, None), 10), ((3, 4, None), 6)])
@pytest.mark.parametrize("cfl", [8.0, 40.0])
def test_unforced_kinetic_energy_never_rises(numpy_engine, grid, steps, cfl):
    """Unforced, from a seeded projected start scaled to tau * CflRate = `cfl`: the symmetric part of N(a) is positive
    semi-definite for the discretely divergence-free a = I_adv u^n, so |u*|_M <= |u^n|_M for any tau and the
    M-orthogonal projection only lowers the energy further.  The reference restatement satisfies the bound on these
    inputs (asserted first); the record of `Advance` must too: never a rise of more than 1e-10 of the start."""
    import hipla
    ns = fresh(grid, treatment="implicit")
    s = ns.system
    ns.f.vec.data = hipla.Vector.from_numpy(np.zeros(s.n_u))
    u0 = ns.gfu.numpy() * (cfl / (TAU * ns.CflRate()))
    ns.gfu.data = hipla.Vector.from_numpy(u0)
    assert TAU * ns.CflRate() == pytest.approx(cfl, rel=1e-12)
    e0 = 0.5 * s.h ** s.dim * float(u0 @ u0)
    _, ref = icr.reference_run(s, u0, np.zeros(s.n_u), [TAU] * steps)
    assert (np.diff(np.concatenate([[e0], ref])) <= 1e-10 * e0).all()
    rec = ns.Advance(steps, **TIGHT)
    energy = np.concatenate([[e0], rec.kinetic_energy])
    print("cfl %g: energy / start %s, iterations %s" % (cfl, energy / e0, rec.mstar_iterations))
    assert (np.diff(energy) <= 1e-10 * e0).all()
    assert np.allclose(rec.kinetic_energy, ref, rtol=1e-8, atol=0.0)


# ---- the C ABI -----------------------------------------------------------------------------------------------------------
def test_bicgstab_state_mirror_matches_the_header(tmp_path):
    """`fused.BicgstabState` against ``nss_bicgstab_t`` field by field (the check tests/test_cabi_symbols.py makes for the
    other loop states), and the entry points in the header, the library's signatures and the Makefile's sources."""
    import ctypes
    import os
    import shutil
    import subprocess
    from conftest import ROOT
    from hipla import fused
    from hipla.hip_engine import _signatures
    from test_cabi_symbols import declared_symbols
    names = [n for n in declared_symbols() if n.startswith("nss_bicgstab_")]
    assert sorted(names) == ["nss_bicgstab_apply_f64", "nss_bicgstab_iterate", "nss_bicgstab_jacobi_f64",
                             "nss_bicgstab_poll", "nss_bicgstab_start", "nss_bicgstab_workspace"]
    assert set(names) <= set(_signatures())
    assert os.path.exists(os.path.join(ROOT, "navier-stokes-solver_amd", "csrc", "bicgstab.hip"))
    cc = next((c for c in (os.environ.get("CC"), "cc", "gcc", "clang") if c and shutil.which(c)), None)
    if cc is None:
        pytest.skip("no C compiler")
    mirror = fused.BicgstabState
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "nss_krylov.h"', "int main(void) {",
             '  printf("- %zu %zu\\n", sizeof(nss_bicgstab_t), _Alignof(nss_bicgstab_t));']
    for fname, _ in mirror._fields_:
        lines.append('  printf("%s %%zu %%zu\\n", offsetof(nss_bicgstab_t, %s), sizeof(((nss_bicgstab_t*)0)->%s));'
                     % (fname, fname, fname))
    lines += ["  return 0;", "}"]
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines) + "\n")
    subprocess.run([cc, "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)],
                   check=True, capture_output=True, text=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split("\n")
    got = {f: (int(a), int(b)) for f, a, b in (line.split() for line in out if line)}
    assert got["-"] == (ctypes.sizeof(mirror), ctypes.alignment(mirror))
    for fname, ftype in mirror._fields_:
        desc = getattr(mirror, fname)
        assert got[fname] == (desc.offset, desc.size) and desc.size == ctypes.sizeof(ftype), fname
    assert {"plan_gen", "cap_a", "cap_b"} <= {f for f, _ in mirror._fields_}
