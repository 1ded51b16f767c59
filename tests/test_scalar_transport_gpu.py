"""`NavierStokes.AddScalar` + `Advance` on the product engine (hipla.fused.ScalarStepper, csrc/scalar.hip): the coupled
device-resident step against tests/scalar_reference.py (direct sparse solves) and against `DoTimeStep` itself, the
passive scalar and the stepper without a scalar against the velocity-only stepper bit for bit.  Tolerances: DESIGN.md
section 3 -- 1e-13 for a kernel against numpy, 1e-9 / 1e-8 behind converged inner solves.

Start field and force are scaled as in tests/test_time_stepper_gpu.py (1e-2 times the projected seeded field, 1e-4 times
the seeded force) and the buoyancy is small enough that |u| timestep / h stays below 0.05 over the five steps (asserted)."""

import contextlib
import io

import numpy as np
import pytest

from oracle import krylov_ref as kr
from scalar_reference import coupled_step

pytestmark = pytest.mark.gpu

TIGHT = dict(precision=1e-14, maxsteps=(5000, 20000))
CASES = {"2d": (2, 8, (0.0, 0.5)), "3d": (3, 5, (0.0, 0.5, -0.2))}
WALLS = {"x-": 1.0, "x+": 0.0}


def rel(a, b):
    return np.linalg.norm(a - b) / np.linalg.norm(b)


def fresh(case, scalar=True, buoyant=True):
    import hipla
    from templates.NavierStokesSIMPLE_iterative import NavierStokes, SyntheticMesh
    dim, n, beta = CASES[case]
    ns = NavierStokes(SyntheticMesh(1.0 / n, dim=dim), nu=0.01, inflow="inlet", outflow="outlet", wall="wall|cyl",
                      uin=None, timestep=0.05, order=0)
    s = ns.system
    assert s.block_size == 1 and s.n == n
    ns.f.vec.data = hipla.Vector.from_numpy(1e-4 * np.random.default_rng(8).standard_normal(s.n_u))
    u0 = 1e-2 * kr.project(s.B, np.full(s.n_u, s.h ** s.dim), np.random.default_rng(2).standard_normal(s.n_u))[0]
    ns.gfu.data = hipla.Vector.from_numpy(u0)
    if scalar:
        ns.AddScalar(0.8, dirichlet=WALLS, buoyancy=beta if buoyant else None, t_ref=0.5,
                     initial=np.random.default_rng(6).random(s.n_p), precision=1e-14, maxsteps=5000)
    return ns


def scalar_args(case, buoyant=True):
    return dict(kappa=0.8, dirichlet=WALLS, buoyancy=CASES[case][2] if buoyant else None, t_ref=0.5)


def tighten(ns):
    """The inner solvers of the statements run to convergence."""
    import hipla
    ops = ns._time_stepping_operators()
    ops["invmstar"] = hipla.CGSolver(ops["mstar"], pre=hipla.JacobiPreconditioner(ops["mstar"]), precision=1e-14, maxsteps=5000)
    ops["invproj"] = hipla.CGSolver(ops["Lp"], pre=hipla.JacobiPreconditioner(ops["Lp"]), precision=1e-14, maxsteps=20000)
    return ns


@pytest.mark.parametrize("inner_pre", ["jacobi", "amg"])
@pytest.mark.parametrize("case", ["2d", "3d"])
def test_one_step_against_the_reference(hip_engine, case, inner_pre):
    """Advance(1) with converged inner solves against `coupled_step`: G, f_eff and temp_T to 1e-13, delta to 1e-9,
    T, u and the recorded wall flux to 1e-8."""
    ns = fresh(case)
    s = ns.system
    u0, T0, f = ns.gfu.numpy(), ns.temperature.numpy(), ns.f.vec.numpy()
    want = coupled_step(s, ns.timestep, u0, T0, f, **scalar_args(case))
    rec = ns.Advance(1, inner_pre=inner_pre, **TIGHT)
    assert rec.declined is None and ns.advance_declined is None and rec.flux_declined is None
    st = ns._scalar.steppers[inner_pre]
    errs = dict(G=rel(hip_engine.to_host(st.G), want["G"]), f_eff=rel(hip_engine.to_host(st.f_eff), want["f_eff"]),
                temp_T=rel(hip_engine.to_host(st.temp), want["temp_T"]), delta=rel(hip_engine.to_host(st.delta), want["delta"]),
                T=rel(ns.temperature.numpy(), want["T"]), u=rel(ns.gfu.numpy(), want["u"]),
                wall=abs(rec.wall_flux[0] - want["wall_flux"]) / abs(want["wall_flux"]))
    print(case, inner_pre, errs, rec.mstar_iterations, rec.proj_iterations, rec.scalar_iterations)
    assert np.linalg.norm(want["f_eff"] - f) > 0.1 * np.linalg.norm(f)          # the buoyancy is visible in the force
    assert errs["G"] < 1e-13 and errs["f_eff"] < 1e-13 and errs["temp_T"] < 1e-13
    assert errs["delta"] < 1e-9
    assert errs["T"] < 1e-8 and errs["u"] < 1e-8 and errs["wall"] < 1e-8
    assert 0 < rec.scalar_iterations[0] < 5000 and rec.wall_flux.shape == (1,)


@pytest.mark.parametrize("case", ["2d", "3d"])
def test_five_steps_against_do_time_step(hip_engine, case):
    """Advance(5) against five `DoTimeStep()` calls on a twin, both with converged solves: T and u to 1e-8; the record
    holds the heat entering through the first Dirichlet wall after every step."""
    ns, twin = fresh(case), tighten(fresh(case))
    rec = ns.Advance(5, **TIGHT)
    walls = []
    with contextlib.redirect_stdout(io.StringIO()):
        for _ in range(5):
            twin.DoTimeStep()
            walls.append(twin._scalar.wall_flux(twin.temperature))
    s = ns.system
    assert np.abs(twin.gfu.numpy()).max() * ns.timestep / s.h < 0.05
    errs = (rel(ns.temperature.numpy(), twin.temperature.numpy()), rel(ns.gfu.numpy(), twin.gfu.numpy()),
            np.abs(rec.wall_flux - np.array(walls)).max() / np.abs(walls).max())
    print(case, errs, rec.scalar_iterations)
    assert rec.declined is None and max(errs) < 1e-8
    assert rec.wall_flux.shape == (5,) and rec.scalar_iterations.shape == (5,) and rec.div_norm.shape == (5,)
    free = fresh(case, scalar=False)                                # the buoyancy moved the fluid
    free.Advance(5, **TIGHT)
    assert rel(free.gfu.numpy(), ns.gfu.numpy()) > 1e-3
    rec = ns.Advance(2, diagnostics=False, **TIGHT)
    assert rec.wall_flux is None and rec.div_norm is None and rec.scalar_iterations.shape == (2,)
    with pytest.raises(ValueError):
        ns.Advance(1, pseudo=True)


@pytest.mark.parametrize("case", ["2d", "3d"])
def test_passive_scalar_leaves_the_velocity_bit_for_bit(hip_engine, case):
    """buoyancy=None: u after Advance(3) is bit for bit what Advance gives without a scalar, while T moves."""
    ns, free = fresh(case, buoyant=False), fresh(case, scalar=False)
    T0 = ns.temperature.numpy()
    rec, rec_free = ns.Advance(3), free.Advance(3)
    assert rec.declined is None and ns._scalar.steppers["jacobi"].f_eff is None
    assert np.array_equal(ns.gfu.numpy(), free.gfu.numpy()) and np.array_equal(ns.gfup.numpy(), free.gfup.numpy())
    assert np.array_equal(rec.kinetic_energy, rec_free.kinetic_energy) and np.array_equal(rec.div_norm, rec_free.div_norm)
    assert np.array_equal(rec.mstar_iterations, rec_free.mstar_iterations)
    assert rel(ns.temperature.numpy(), T0) > 1e-3 and rec.wall_flux.shape == (3,)
    assert rec_free.wall_flux is None and rec_free.scalar_iterations is None


def test_uniform_reference_temperature_exerts_no_force(hip_engine):
    """A buoyant scalar at T = t_ref everywhere: f_eff == f exactly, so the first step moves u bit for bit as without a
    scalar (afterwards the walls have heated the fluid)."""
    ns, free = fresh("2d", scalar=False), fresh("2d", scalar=False)
    ns.AddScalar(0.8, dirichlet=WALLS, buoyancy=(0.3, 0.5), t_ref=0.5)
    rec = ns.Advance(1)
    free.Advance(1)
    st = ns._scalar.steppers["jacobi"]
    assert rec.declined is None and np.array_equal(hip_engine.to_host(st.f_eff), ns.f.vec.numpy())
    assert np.array_equal(ns.gfu.numpy(), free.gfu.numpy())
    assert np.abs(ns.temperature.numpy() - 0.5).max() > 1e-3


def test_without_a_scalar_nothing_changes_and_nothing_leaks(hip_engine):
    """Without `AddScalar` the stepper takes the velocity-only path: Advance(3) on an object that never saw a scalar and
    on one created after ANOTHER object's AddScalar + Advance give the same bits (record included), and so does a
    second run of either -- no state is shared between objects."""
    def run():
        ns = fresh("2d", scalar=False)
        rec = ns.Advance(3)
        assert rec.declined is None and rec.scalar_iterations is None and rec.wall_flux is None
        assert ns._scalar is None and not hasattr(ns, "temperature")
        return ns.gfu.numpy(), ns.gfup.numpy(), rec.kinetic_energy, rec.div_norm, rec.mstar_iterations, rec.proj_iterations

    before = run()
    other = fresh("2d")
    other.Advance(2)
    after = run()
    for a, b in zip(before, after):
        assert np.array_equal(a, b)
    assert rel(other.gfu.numpy(), after[0]) > 1e-6                  # (the scalar run itself was a different flow)
