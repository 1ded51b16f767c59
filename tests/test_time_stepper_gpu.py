"""`NavierStokes.Advance` (hipla.fused.TimeStepper, csrc/step.hip) on the product engine: the device-resident IMEX step
against the oracle's statement-by-statement `do_time_step` / `project` (direct sparse solves) and against `DoTimeStep` /
`SolveInitial(timesteps=)` themselves.  The system is that of test_hip_solvers.py::test_time_stepping_on_gpu; the
tolerances are those of DESIGN.md section 3 (1e-13 for a kernel against numpy, 1e-9 / 1e-8 for converged inner solves)."""

import contextlib
import io

import numpy as np
import pytest
import scipy.sparse as sp

from oracle import krylov_ref as kr

pytestmark = pytest.mark.gpu

TIGHT = dict(precision=1e-14, maxsteps=(5000, 20000))


def rel(a, b):
    return np.linalg.norm(a - b) / np.linalg.norm(b)


def fresh(dim=3, maxh=0.1):
    import hipla  # noqa: F401
    from templates.NavierStokesSIMPLE_iterative import NavierStokes, SyntheticMesh
    ns = NavierStokes(SyntheticMesh(maxh, dim=dim), nu=0.01, inflow="inlet", outflow="outlet", wall="wall|cyl", uin=None,
                      timestep=0.05, order=1)
    ns.AddForce(np.random.default_rng(8).standard_normal(ns.system.n_u))
    return ns


def mass_of(s):
    return np.full(s.n_u, s.h ** s.dim)


def start_velocity(s):
    """The oracle's projection of a seeded field."""
    return kr.project(s.B, mass_of(s), np.random.default_rng(2).standard_normal(s.n_u))[0]


def oracle_step(ns, u0):
    s = ns.system
    cops = s.convection_operators()
    return kr.do_time_step(s.A, s.B, mass_of(s), ns.timestep, u0, ns.f.vec.numpy(), lambda u: kr.upwind_convection(cops, u))


def tighten(ns):
    """The inner solvers of the statements run to convergence, as in test_time_stepping_on_gpu."""
    import hipla
    ops = ns._time_stepping_operators()
    ops["invmstar"] = hipla.CGSolver(ops["mstar"], pre=hipla.JacobiPreconditioner(ops["mstar"]), precision=1e-14, maxsteps=5000)
    ops["invproj"] = hipla.CGSolver(ops["Lp"], pre=hipla.JacobiPreconditioner(ops["Lp"]), precision=1e-14, maxsteps=20000)
    return ns


def set_velocity(ns, u):
    import hipla
    ns.gfu.data = hipla.Vector.from_numpy(u)


@pytest.mark.parametrize("case", ["3d-inflated", "2d-inflated", "2d-plain", "3d-plain"])
def test_flux_and_right_hand_side_against_numpy(hip_engine, case):
    """The F part of [u | F] equals adv*avg - |adv| diff / 2 and temp equals the oracle's temp, both to 1e-13: plain
    systems and inflated ones (block_size > 1: the operators (x) I through the same kernels)."""
    import hipla
    from hipla.fused import TimeStepper
    from staggered_grid import mac_stokes
    dim = int(case[0])
    s = mac_stokes(dim, 9 if dim == 3 else 14, 0.01)
    if case.endswith("inflated"):
        s = s.inflate(3)
    assert (s.block_size > 1) == case.endswith("inflated")
    A, B = hipla.SparseMatrix.from_scipy(s.A), hipla.SparseMatrix.from_scipy(s.B)
    f = np.random.default_rng(8).standard_normal(s.n_u)
    st = TimeStepper.try_create(s, A, B, hipla.Vector.from_numpy(f), 0.05, mass_of(s))
    assert st is not None and st.flux_declined is None, (TimeStepper.last_declined, st and st.flux_declined)
    u0 = np.random.default_rng(2).standard_normal(s.n_u)
    hip_engine.upload(u0, st.u)
    st.right_hand_side()
    cops = s.convection_operators()
    adv, avg, dif = cops["adv"] @ u0, cops["avg"] @ u0, cops["diff"] @ u0
    want_flux = adv * avg - 0.5 * np.abs(adv) * dif
    got = hip_engine.to_host(st.uf)
    assert np.array_equal(got[:s.n_u], u0)
    err_flux = rel(got[s.n_u:], want_flux)
    want = kr.do_time_step(s.A, s.B, mass_of(s), 0.05, u0, f, lambda u: kr.upwind_convection(cops, u))["temp"]
    err_temp = rel(hip_engine.to_host(st.temp), want)
    print("flux", err_flux, "temp", err_temp)
    assert err_flux < 1e-13
    assert err_temp < 1e-13


@pytest.mark.parametrize("dim", [3, 2])
@pytest.mark.parametrize("inner_pre", ["jacobi", "amg"])
def test_one_step_against_the_oracle(hip_engine, dim, inner_pre):
    """Advance(1) with converged inner solves against `kr.do_time_step`: unprojected increment 1e-9, projected
    increment and new velocity 1e-8."""
    ns = fresh(dim)
    u0 = start_velocity(ns.system)
    want = oracle_step(ns, u0)
    set_velocity(ns, u0)
    rec = ns.Advance(1, inner_pre=inner_pre, **TIGHT)
    assert rec.declined is None and ns.advance_declined is None and rec.flux_declined is None
    st = ns._steppers[inner_pre]
    errs = (rel(hip_engine.to_host(st.temp), want["temp"]), rel(hip_engine.to_host(st.raw), want["temp2_unprojected"]),
            rel(hip_engine.to_host(st.temp2), want["temp2"]), rel(ns.gfu.numpy(), want["u"]))
    print(inner_pre, dim, errs, rec.mstar_iterations, rec.proj_iterations)
    assert errs[0] < 1e-13
    assert errs[1] < 1e-9
    assert errs[2] < 1e-8
    assert errs[3] < 1e-8
    assert rec.mstar_iterations[0] < 5000 and rec.proj_iterations[0] < 20000


@pytest.mark.parametrize("inner_pre", ["jacobi", "amg"])
def test_one_step_with_non_uniform_mass(hip_engine, inner_pre):
    """One `advance` of a `TimeStepper` made with a NON-uniform lumped mass m_u = h^2 (0.5 + random) -- the `mass`
    operand of the projection launch, energy_scale = 0.5 -- against `kr.do_time_step` with the same m_u: the bounds of
    test_one_step_against_the_oracle; kinetic_energy[0] = u . (m_u u) / 2 to 1e-12, visibly not h^2 |u|^2 / 2."""
    from math import fsum
    import hipla
    from hipla.fused import TimeStepper
    from staggered_grid import mac_stokes
    s = mac_stokes(2, 14, 0.01)
    rng = np.random.default_rng(14)
    m_u = s.h ** 2 * (0.5 + rng.random(s.n_u))
    f = np.random.default_rng(8).standard_normal(s.n_u)
    A, B = hipla.SparseMatrix.from_scipy(s.A), hipla.SparseMatrix.from_scipy(s.B)
    st = TimeStepper.try_create(s, A, B, hipla.Vector.from_numpy(f), 0.05, m_u, inner_pre=inner_pre)
    assert st is not None and st.flux_declined is None, (TimeStepper.last_declined, st and st.flux_declined)
    assert st.mass is not None and st.energy_scale == 0.5
    assert np.array_equal(hip_engine.to_host(st.mass), m_u)
    u0 = kr.project(s.B, m_u, np.random.default_rng(2).standard_normal(s.n_u))[0]
    cops = s.convection_operators()
    want = kr.do_time_step(s.A, s.B, m_u, 0.05, u0, f, lambda u: kr.upwind_convection(cops, u))
    gfu, gfup = hipla.Vector.from_numpy(u0), hipla.Vector(s.n_p)
    rec = st.advance(gfu, gfup, 1, **TIGHT)
    u = gfu.numpy()
    errs = (rel(hip_engine.to_host(st.temp), want["temp"]), rel(hip_engine.to_host(st.raw), want["temp2_unprojected"]),
            rel(hip_engine.to_host(st.temp2), want["temp2"]), rel(u, want["u"]))
    energy, unweighted = 0.5 * fsum(u * (m_u * u)), 0.5 * s.h ** 2 * fsum(u * u)
    print(inner_pre, errs, rec.mstar_iterations, rec.proj_iterations, "energy", rec.kinetic_energy[0], energy, unweighted)
    assert errs[0] < 1e-13
    assert errs[1] < 1e-9
    assert errs[2] < 1e-8
    assert errs[3] < 1e-8
    assert rec.mstar_iterations[0] < 5000 and rec.proj_iterations[0] < 20000
    assert abs(rec.kinetic_energy[0] - energy) <= 1e-12 * energy
    assert abs(unweighted - energy) > 1e-3 * energy


@pytest.mark.parametrize("inner_pre", ["jacobi", "amg"])
def test_default_precision(hip_engine, inner_pre):
    """With the reference's inner precision the step agrees with the oracle to 1e-4 and |B u| obeys the bound of
    test_time_stepping_on_gpu."""
    ns = fresh()
    s = ns.system
    u0 = start_velocity(s)
    want = oracle_step(ns, u0)
    set_velocity(ns, u0)
    rec = ns.Advance(1, inner_pre=inner_pre)
    u = ns.gfu.numpy()
    print(inner_pre, rel(u, want["u"]), np.linalg.norm(s.B @ u), rec.div_norm)
    assert rel(u, want["u"]) < 1e-4
    assert np.linalg.norm(s.B @ u) < 1e-5 * np.linalg.norm(u) * abs(s.B).max()


def damp(ns):
    """The seeded force scaled by 1e-4, for runs of several steps (with the 1e-2 start field of their callers): with the
    N(0, 1) force -- acceleration f / m_u ~ 1e3 -- the explicit convection term at timestep 0.05 overflows after eight
    steps, for the oracle's `do_time_step` with direct solves as well (CPU: |u| 4.5e3, 1.7e5, 3.3e8, 2.3e15, ... inf,
    nan).  Damped, |u| timestep / h stays below 0.05 (|u|_max 0.036 -> 0.087 over eleven oracle steps)."""
    import hipla
    ns.f.vec.data = hipla.Vector.from_numpy(1e-4 * ns.f.vec.numpy())
    return ns


def test_five_steps_against_do_time_step(hip_engine):
    """Advance(5) and five DoTimeStep() calls on a twin, both with converged inner solves: velocities agree to 1e-8;
    Advance(3, pseudo=True) agrees the same way with SolveInitial(timesteps=3).  The five steps run on the damped
    system (`damp`), a trajectory that stays bounded."""
    ns, twin = damp(fresh()), tighten(damp(fresh()))
    u0 = 1e-2 * start_velocity(ns.system)
    set_velocity(ns, u0)
    set_velocity(twin, u0)
    rec = ns.Advance(5, **TIGHT)
    with contextlib.redirect_stdout(io.StringIO()):
        for _ in range(5):
            twin.DoTimeStep()
    err = rel(ns.gfu.numpy(), twin.gfu.numpy())
    print("five steps", err, rec.mstar_iterations, rec.proj_iterations, np.abs(ns.gfu.numpy()).max())
    assert np.abs(ns.gfu.numpy()).max() < 1.0
    assert err < 1e-8
    assert rel(ns.gfup.numpy(), twin.gfup.numpy()) < 1e-6        # (the potential of the last projection, for the record)

    ns, twin = fresh(), tighten(fresh())
    v0 = np.random.default_rng(2).standard_normal(ns.system.n_u)
    set_velocity(ns, v0)
    set_velocity(twin, v0)
    rec = ns.Advance(3, pseudo=True, **TIGHT)
    with contextlib.redirect_stdout(io.StringIO()):
        twin.SolveInitial(timesteps=3)
    err = rel(ns.gfu.numpy(), twin.gfu.numpy())
    print("pseudo", err, rec.mstar_iterations, rec.proj_iterations)
    assert err < 1e-8
    assert len(rec.mstar_iterations) == len(rec.proj_iterations) == len(rec.div_norm) == 3


def test_enclosed_domain_amg_and_unchanged_default(hip_engine):
    """The all-wall cavity: the pressure operator has the constants in its kernel (the oracle's own test); the AMG
    projection with nullspace="constants" gives finite values and agrees with `kr.project` (which pins one pressure) to
    1e-8.  Without `nullspace` a V-cycle on a non-singular operator is bit for bit what nullspace=None gives, and an
    AMG-preconditioned solve takes the same iterations."""
    import hipla
    ns = fresh()
    s = ns.system
    m_u = mass_of(s)
    L = (s.B @ (sp.diags(1.0 / m_u) @ s.B.T)).tocsr()
    assert np.linalg.norm(L @ np.ones(L.shape[0])) <= 1e-12 * abs(L).sum()
    u0 = start_velocity(s)
    want = oracle_step(ns, u0)
    set_velocity(ns, u0)
    rec = ns.Advance(1, inner_pre="amg", **TIGHT)
    st = ns._steppers["amg"]
    assert st.singular and st.pre_p.nullspace == "constants" and st.pre_m.nullspace is None
    assert np.isfinite(ns.gfu.numpy()).all() and np.isfinite(ns.gfup.numpy()).all()
    assert np.isfinite(rec.div_norm).all() and np.isfinite(rec.kinetic_energy).all()
    vel = np.random.default_rng(5).standard_normal(s.n_u)
    hip_engine.upload(vel, st.raw)
    st.project(st.raw, out=st.temp2)
    got = hip_engine.to_host(st.temp2)
    ref_v, _ = kr.project(s.B, m_u, vel)
    print("project", rel(got, ref_v), "step", rel(ns.gfu.numpy(), want["u"]))
    assert rel(got, ref_v) < 1e-8
    assert rel(ns.gfu.numpy(), want["u"]) < 1e-8

    mstar = st.mstar                                                      # non-singular: M_u + tau A
    plain, explicit = hipla.SmoothedAggregationAMG(mstar), hipla.SmoothedAggregationAMG(mstar, nullspace=None)
    x = hipla.Vector.from_numpy(np.random.default_rng(6).standard_normal(s.n_u))
    ya, yb = x.CreateVector(), x.CreateVector()
    ya.data = plain * x
    yb.data = explicit * x
    assert np.array_equal(ya.numpy(), yb.numpy())
    for lv_a, lv_b in zip(plain.levels, explicit.levels):
        assert lv_a["n"] == lv_b["n"]
    assert np.array_equal(plain.levels[-1]["inv"].to_scipy().toarray(), explicit.levels[-1]["inv"].to_scipy().toarray())
    assert np.array_equal(plain.levels[-1]["inv"].to_scipy().toarray(),
                          np.linalg.inv(plain.levels[-1]["A"].to_scipy().toarray()))       # the inverse, as before
    counts = []
    for pre in (plain, explicit):
        solver = hipla.CGSolver(mstar, pre=pre, precision=1e-10, maxsteps=500)
        y = x.CreateVector()
        y.data = solver * x
        counts.append((solver.iterations, tuple(solver.errors)))
    assert counts[0] == counts[1]


def test_amg_beats_jacobi_on_iterations(hip_engine):
    """Iteration counts, not time: on 3-D grids with >= 24 cells per side the AMG-preconditioned projection takes
    strictly fewer iterations than the Jacobi one in every step, and from n = 16 to n = 32 its count grows by less than
    Jacobi's does (CPU check of the premise with kr.cg + Jacobi on B M_u^-1 B^T of these systems: 87 -> 172)."""
    counts = {}
    for n in (16, 24, 32):
        ns = fresh(3, 1.0 / n)
        assert ns.system.n == n
        v0 = np.random.default_rng(2).standard_normal(ns.system.n_u)
        for inner_pre in ("jacobi", "amg"):
            set_velocity(ns, v0)
            rec = ns.Advance(2, inner_pre=inner_pre)
            assert rec.declined is None
            counts[(n, inner_pre)] = rec.proj_iterations
            print(n, inner_pre, "proj", rec.proj_iterations, "mstar", rec.mstar_iterations)
    for n in (24, 32):
        assert (counts[(n, "amg")] < counts[(n, "jacobi")]).all(), (n, counts)
    growth = {pre: counts[(32, pre)].max() - counts[(16, pre)].max() for pre in ("jacobi", "amg")}
    assert growth["jacobi"] > 0 and growth["amg"] < growth["jacobi"], (growth, counts)


def test_allocations_and_records(hip_engine):
    """No allocation survives a second Advance; the record arrays have one entry per step; div_norm and kinetic_energy
    equal |B u| and u^T M_u u / 2 recomputed in numpy from the final state to 1e-12; diagnostics=False leaves them None
    and the velocities identical.

    Eleven steps are taken here.  With the seeded N(0, 1) force (acceleration f / m_u ~ 1e3) the explicit convection
    term at timestep 0.05 overflows after eight steps -- for the oracle's `do_time_step` with direct solves as well (CPU:
    |u| 4.5e3, 1.7e5, 3.3e8, 2.3e15, ... inf, nan) -- so there is no finite last step to compare.  Same system, same
    seeds, force scaled by 1e-4 and start field by 1e-2 (|u| timestep / h < 0.05 throughout: |u|_max 0.036 -> 0.087 over
    the eleven oracle steps); the step counts and the 1e-12 bounds stay."""
    import hipla
    import torch
    ns, quiet = fresh(), fresh()
    s = ns.system
    for twin in (ns, quiet):
        damp(twin)
    u0 = 1e-2 * start_velocity(s)
    set_velocity(ns, u0)
    set_velocity(quiet, u0)
    ns.Advance(1)
    quiet.Advance(1, diagnostics=False)
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    rec = ns.Advance(10)
    torch.cuda.synchronize()
    assert torch.cuda.memory_allocated() == before          # (the record is host memory)
    for arr in (rec.mstar_iterations, rec.proj_iterations, rec.div_norm, rec.kinetic_energy):
        assert len(arr) == 10
    u = ns.gfu.numpy()
    div, energy = np.linalg.norm(s.B @ u), 0.5 * float(u @ (mass_of(s) * u))
    print("div", rec.div_norm[-1], div, "energy", rec.kinetic_energy[-1], energy)
    assert abs(rec.kinetic_energy[-1] - energy) <= 1e-12 * energy
    assert abs(rec.div_norm[-1] - div) <= 1e-12 * div
    bare = quiet.Advance(10, diagnostics=False)
    assert bare.div_norm is None and bare.kinetic_energy is None and len(bare.proj_iterations) == 10
    assert np.array_equal(quiet.gfu.numpy(), u)
    assert np.array_equal(bare.proj_iterations, rec.proj_iterations)


def test_decline_path(hip_engine):
    """With the fused loops switched off Advance runs the statements: the velocity of two DoTimeStep() calls, and a reason."""
    import hipla.fused
    ns, twin = fresh(), fresh()
    u0 = start_velocity(ns.system)
    set_velocity(ns, u0)
    set_velocity(twin, u0)
    prev = hipla.fused.ENABLED
    hipla.fused.ENABLED = False
    try:
        rec = ns.Advance(2)
        with contextlib.redirect_stdout(io.StringIO()):
            twin.DoTimeStep()
            twin.DoTimeStep()
    finally:
        hipla.fused.ENABLED = prev
    assert rec.declined and ns.advance_declined == rec.declined
    assert np.array_equal(ns.gfu.numpy(), twin.gfu.numpy())
    assert len(rec.mstar_iterations) == len(rec.proj_iterations) == len(rec.div_norm) == len(rec.kinetic_energy) == 2
    rec = ns.Advance(1)                                     # switched on again: the device-resident step
    assert rec.declined is None and ns.advance_declined is None


# ---- Advance(0): no step, and everything around the loop ------------------------------------------------------------
RECORD_ARRAYS = ("mstar_iterations", "proj_iterations", "div_norm", "kinetic_energy", "scalar_iterations", "wall_flux")


def small(scalar=None):
    """The 2-D grid of tests/test_limited_convection_gpu.py::fresh_scalar("2d") (n = 8, a plain system), damped the same
    way.  `scalar`: None, "wall" (a buoyant scalar whose Dirichlet wall is recorded) or "no wall" (buoyant, insulated)."""
    import hipla
    from templates.NavierStokesSIMPLE_iterative import NavierStokes, SyntheticMesh
    ns = NavierStokes(SyntheticMesh(1.0 / 8, dim=2), nu=0.01, inflow="inlet", outflow="outlet", wall="wall|cyl", uin=None,
                      timestep=0.05, order=0)
    s = ns.system
    assert s.block_size == 1 and s.n == 8
    ns.f.vec.data = hipla.Vector.from_numpy(1e-4 * np.random.default_rng(8).standard_normal(s.n_u))
    set_velocity(ns, 1e-2 * start_velocity(s))
    if scalar is not None:
        ns.AddScalar(0.8, dirichlet={"x-": 1.0, "x+": 0.0} if scalar == "wall" else None, buoyancy=(0.0, 0.5), t_ref=0.5,
                     initial=np.random.default_rng(6).random(s.n_p))
    return ns


def mark_potential(ns):
    """A seeded, non-zero gfup: what a call that must not write it leaves bit for bit."""
    import hipla
    ns.gfup.data = hipla.Vector.from_numpy(np.random.default_rng(11).standard_normal(ns.system.n_p))
    return ns.gfup.numpy().copy()


def check_empty_record(rec, one, diagnostics, scalar):
    """`rec` of Advance(0) against `one` of Advance(1) on the same object: empty arrays of the same dtypes, None where
    `one` holds None -- and that is where it must: the diagnostics without `diagnostics`, the scalar's arrays without a
    scalar, the wall flux without a flux wall."""
    assert rec.declined is None and one.declined is None
    for name in RECORD_ARRAYS:
        got, ref = getattr(rec, name), getattr(one, name)
        if ref is None:
            assert got is None, name
        else:
            assert isinstance(got, np.ndarray) and got.shape == (0,) and got.dtype == ref.dtype and ref.shape == (1,), name
    assert (one.div_norm is None) == (one.kinetic_energy is None) == (not diagnostics)
    assert (one.scalar_iterations is None) == (scalar is None)
    assert (one.wall_flux is None) == (scalar != "wall" or not diagnostics)


@pytest.mark.parametrize("diagnostics", [True, False])
@pytest.mark.parametrize("grid", ["2d", "3d"])
def test_advance_zero_steps(hip_engine, grid, diagnostics):
    """Advance(0) without a scalar: gfu and gfup bit-unchanged, the record's arrays empty with the dtypes of Advance(1),
    div_norm and kinetic_energy None with diagnostics=False."""
    ns = small() if grid == "2d" else fresh()
    if grid == "3d":
        set_velocity(ns, start_velocity(ns.system))
    u0, p0 = ns.gfu.numpy().copy(), mark_potential(ns)
    rec = ns.Advance(0, diagnostics=diagnostics)
    assert np.array_equal(ns.gfu.numpy(), u0) and np.array_equal(ns.gfup.numpy(), p0)
    check_empty_record(rec, ns.Advance(1, diagnostics=diagnostics), diagnostics, None)


@pytest.mark.parametrize("scalar,diagnostics", [("wall", True), ("wall", False), ("no wall", True)])
def test_advance_zero_steps_with_a_buoyant_scalar(hip_engine, scalar, diagnostics):
    """Advance(0) with a buoyant scalar: gfu, gfup and the temperature bit-unchanged; scalar_iterations and wall_flux
    empty as well, wall_flux None without a flux wall (and without diagnostics)."""
    ns = small(scalar)
    u0, p0, T0 = ns.gfu.numpy().copy(), mark_potential(ns), ns.temperature.numpy().copy()
    rec = ns.Advance(0, diagnostics=diagnostics)
    assert np.array_equal(ns.gfu.numpy(), u0) and np.array_equal(ns.gfup.numpy(), p0)
    assert np.array_equal(ns.temperature.numpy(), T0)
    one = ns.Advance(1, diagnostics=diagnostics)
    check_empty_record(rec, one, diagnostics, scalar)
    assert not np.array_equal(ns.temperature.numpy(), T0)           # (the scalar is live: one step moves it)


@pytest.mark.parametrize("grid", ["2d", "3d"])
def test_advance_zero_pseudo_steps_project(hip_engine, grid):
    """Advance(0, pseudo=True) is the leading Project(gfu) of the pseudo time stepping: gfu agrees with `Project` on a
    twin to 1e-8 (both with converged solves, the bound and the twin of test_five_steps_against_do_time_step), gfup is
    written, the record is empty."""
    ns, twin = (small(), tighten(small())) if grid == "2d" else (fresh(), tighten(fresh()))
    v0 = np.random.default_rng(2).standard_normal(ns.system.n_u)
    set_velocity(ns, v0)
    set_velocity(twin, v0)
    p0 = mark_potential(ns)
    rec = ns.Advance(0, pseudo=True, **TIGHT)
    twin.Project(twin.gfu)
    err = rel(ns.gfu.numpy(), twin.gfu.numpy())
    print("pseudo, no step", grid, err, rel(ns.gfup.numpy(), twin.gfup.numpy()))
    assert err < 1e-8
    assert rel(ns.gfu.numpy(), v0) > 1e-2                            # (the projection moved the field)
    assert not np.array_equal(ns.gfup.numpy(), p0) and np.isfinite(ns.gfup.numpy()).all()
    check_empty_record(rec, ns.Advance(1, pseudo=True, **TIGHT), True, None)
