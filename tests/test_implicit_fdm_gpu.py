"""`NavierStokes.SetImplicitSolve("fdm")` on the product engine: the device-resident stepper and the statements with the
direct velocity and scalar solves against a twin left at "cg" whose solves run to 1e-12 (velocity), 1e-13 (projection)
and 1e-14 (scalar).

Bounds.  1e-9 relative on the velocity, the potential (mean removed: the constants are in the kernel of the pressure
operator) and the temperature: the bound the project uses for such twins (tests/test_fdm_gpu.py), whose own CG error it
is -- the direct solves err at rounding level.  The twin takes the same projection as the object under test, so that the
implicit solves are what differs.  Bit-for-bit where the same launches run: split calls, and an object back at "cg"."""

import contextlib
import io

import numpy as np
import pytest

from oracle import krylov_ref as kr

pytestmark = pytest.mark.gpu

TAU = 0.05
WALLS = {"x-": 1.0, "x+": 0.0}
GRIDS = {"2d": (2, 8, (0.0, 2.0)), "3d": (3, 5, (0.0, 2.0, -1.0))}
SIZES = [0.05, 0.03, 0.045, 0.02]
TIGHT = dict(precision=(1e-12, 1e-13))
# The pseudo time stepping projects velocities that are divergence-free already: B u is rounding noise with a component
# along the constants, on which a CG projection never reaches a relative 1e-13 and runs to its cap, losing digits of u
# with every iteration (tests/test_fdm_gpu.py; with the default cap of 5000 two "cg"-projection objects measured 2.3e-9
# apart in 2-D).  A projection of these grids takes 31 or 32 iterations (same file): the cap is ten times that, for
# both objects alike.
PSEUDO_CAP = 320
MODES = {"fixed": lambda k: {}, "timesteps": lambda k: dict(timesteps=SIZES[k]), "cfl": lambda k: dict(cfl=0.08),
         "pseudo": lambda k: dict(pseudo=True, maxsteps=(5000, PSEUDO_CAP))}


def fresh(grid, scheme="euler", buoyant=False, projection=None, implicit=None):
    """The set-up of tests/test_fdm_gpu.py: a seeded divergence-free start (max |u| tau / h about 0.1), a seeded force
    and start pressure, optionally a buoyant scalar; `projection` / `implicit`: what `SetProjection` / `SetImplicitSolve`
    are called with (None: not called)."""
    import hipla
    from templates.NavierStokesSIMPLE_iterative import NavierStokes, SyntheticMesh
    dim, n, beta = GRIDS[grid]
    ns = NavierStokes(SyntheticMesh(1.0 / n, dim=dim), nu=0.01, inflow="inlet", outflow="outlet", wall="wall|cyl",
                      uin=None, timestep=TAU, order=0, time_scheme=scheme)
    s = ns.system
    assert s.block_size == 1 and s.n == n
    ns.f.vec.data = hipla.Vector.from_numpy(0.5 * s.h ** s.dim * np.random.default_rng(8).standard_normal(s.n_u))
    u0 = 0.2 * kr.project(s.B, np.full(s.n_u, s.h ** s.dim), np.random.default_rng(2).standard_normal(s.n_u))[0]
    ns.gfu.data = hipla.Vector.from_numpy(u0)
    p0 = np.random.default_rng(4).standard_normal(s.n_p)
    ns.gfup.data = hipla.Vector.from_numpy(0.01 * (p0 - p0.mean()))
    if buoyant:
        ns.AddScalar(initial=np.random.default_rng(6).random(s.n_p), precision=1e-14, maxsteps=5000, kappa=0.8,
                     dirichlet=WALLS, buoyancy=beta, t_ref=0.5)
    if projection is not None:
        ns.SetProjection(projection)
    if implicit is not None:
        ns.SetImplicitSolve(implicit)
    return ns


def rel(a, b):
    return np.linalg.norm(np.asarray(a) - b) / np.linalg.norm(b)


def state(ns):
    out = [ns.gfu.numpy().copy(), ns.gfup.numpy().copy()]
    return out + ([ns.temperature.numpy().copy()] if ns._scalar is not None else [])


def assert_close(direct, twin, what="", pseudo=False):
    """Velocity, potential without its mean, temperature: 1e-9 relative.  `pseudo`: the potential is not compared.  What
    a pseudo time step leaves in `gfup` is the potential of its last projection, of a velocity that is divergence-free
    already: phi = Lp^-1 (rounding noise), which has no digits (measured between two correct runs: |p - q| / |q| of 1
    to 9e5, and as a velocity correction |M_u^-1 B^T (p - q)| / |u| up to 2.4e-9 with the CG projection, 1e-16 with the
    direct one).  The velocity, which every earlier potential of the run has acted on, is compared as ever."""
    errs = [rel(direct.gfu.numpy(), twin.gfu.numpy())]
    p, q = direct.gfup.numpy(), twin.gfup.numpy()
    if not pseudo:
        errs.append(rel(p - p.mean(), q - q.mean()))
    if twin._scalar is not None:
        errs.append(rel(direct.temperature.numpy(), twin.temperature.numpy()))
    print("%s: relative differences (u, gfup, T) %s" % (what, ["%.3g" % e for e in errs]))
    assert max(errs) <= 1e-9, errs


def tighten_statements(ns):
    """The CG solvers of `DoTimeStep` at the precisions of `TIGHT` (the scalar's is set by `AddScalar`)."""
    ops = ns._time_stepping_operators()
    ops["invmstar"].precision, ops["invmstar"].maxsteps = 1e-12, 5000
    if ns.projection == "cg":
        ops["invproj"].precision, ops["invproj"].maxsteps = 1e-13, 20000
    if ns.time_scheme == "cnab2":
        half = ns._cnab2_operators()
        half["invmhalf"].precision, half["invmhalf"].maxsteps = 1e-12, 5000


def quiet(call, *args, **kw):
    with contextlib.redirect_stdout(io.StringIO()):
        return call(*args, **kw)


CASES = [(grid, scheme, buoyant, mode, projection) for grid in sorted(GRIDS) for scheme in ("euler", "cnab2")
         for buoyant in (False, True) for mode in sorted(MODES) for projection in ("cg", "fdm")
         if not (mode == "pseudo" and buoyant)]


@pytest.mark.parametrize("grid,scheme,buoyant,mode,projection", CASES)
def test_advance_against_the_cg_twin(hip_engine, grid, scheme, buoyant, mode, projection):
    direct, twin = fresh(grid, scheme, buoyant, projection, "fdm"), fresh(grid, scheme, buoyant, projection)
    kw = MODES[mode](slice(0, 4))
    rec = direct.Advance(4, **kw, **TIGHT)
    ref = twin.Advance(4, **kw, **TIGHT)
    assert direct.advance_declined is None and twin.advance_declined is None
    assert rec.implicit == "fdm" and ref.implicit == "cg" and rec.projection == ref.projection == projection
    assert rec.mstar_iterations.shape == (4,) and (rec.mstar_iterations == 0).all() and (ref.mstar_iterations > 0).all()
    if buoyant:
        assert (rec.scalar_iterations == 0).all() and (ref.scalar_iterations > 0).all()
    else:
        assert rec.scalar_iterations is None
    assert rec.time_scheme == ("euler" if mode == "pseudo" else scheme)
    if mode in ("timesteps", "cfl"):
        assert np.allclose(rec.timestep, ref.timestep, rtol=1e-9, atol=0.0)
    assert_close(direct, twin, "%s %s buoyant=%s %s projection=%s" % (grid, scheme, buoyant, mode, projection),
                 pseudo=mode == "pseudo")


@pytest.mark.parametrize("scheme", ["euler", "cnab2"])
@pytest.mark.parametrize("variable", [False, True])
def test_a_stepper_with_both_switches_holds_no_iterative_solver(hip_engine, scheme, variable):
    ns = fresh("3d", scheme, True, "fdm", "fdm")
    ns.Advance(2, inner_pre="amg", **(dict(timesteps=SIZES[:2]) if variable else {}))
    assert ns.advance_declined is None and len(ns._steppers) == 1
    stepper = next(iter(ns._steppers.values()))
    for name in ("cg_m", "pre_m", "cg_p", "pre_p", "mstar"):
        assert getattr(stepper, name) is None, name
    assert stepper.fdm_u is ns._fdm_u and ns._stepper_shared["fdm_u"] is ns._fdm_u and stepper.implicit == "fdm"
    (scalar,) = ns._scalar.steppers.values()
    assert scalar.cg is None and scalar.pre is None and scalar.mstar is None
    assert scalar.fdm is ns._scalar.shared["fdm_T"] and not ns._by_step and not ns._scalar.by_step


def test_variable_steps_take_amg_with_the_direct_solve(hip_engine):
    direct, twin = fresh("2d", "euler", True, None, "fdm"), fresh("2d", "euler", True)
    rec = direct.Advance(2, timesteps=SIZES[:2], inner_pre="amg", **TIGHT)
    assert direct.advance_declined is None and rec.implicit == "fdm" and (rec.proj_iterations > 0).all()
    twin.Advance(2, timesteps=SIZES[:2], **TIGHT)
    assert_close(direct, twin, "variable steps, inner_pre=amg")
    with pytest.raises(ValueError):
        twin.Advance(2, timesteps=SIZES[:2], inner_pre="amg")
    direct.SetImplicitSolve("cg")
    with pytest.raises(ValueError):
        direct.Advance(2, timesteps=SIZES[:2], inner_pre="amg")


@pytest.mark.parametrize("scheme", ["euler", "cnab2"])
@pytest.mark.parametrize("mode", ["fixed", "timesteps"])
@pytest.mark.parametrize("projection", ["cg", "fdm"])
def test_split_advance_is_bit_identical(hip_engine, scheme, mode, projection):
    one, two = fresh("2d", scheme, True, projection, "fdm"), fresh("2d", scheme, True, projection, "fdm")
    kw = MODES[mode]
    rec = one.Advance(4, **kw(slice(0, 4)))
    first, second = two.Advance(2, **kw(slice(0, 2))), two.Advance(2, **kw(slice(2, 4)))
    for a, b in zip(state(one), state(two)):
        assert np.array_equal(a, b)
    for name in ("div_norm", "kinetic_energy", "wall_flux", "proj_iterations"):
        assert np.array_equal(getattr(rec, name), np.concatenate([getattr(first, name), getattr(second, name)])), name


@pytest.mark.parametrize("scheme", ["euler", "cnab2"])
def test_do_time_step_and_advance_mix(hip_engine, scheme):
    direct, twin = fresh("3d", scheme, True, "fdm", "fdm"), fresh("3d", scheme, True, "fdm")
    tighten_statements(twin)
    for ns in (direct, twin):
        quiet(ns.DoTimeStep)
        ns.Advance(2, **TIGHT)
        quiet(ns.DoTimeStep, 0.03)
        ns.Advance(1, timesteps=[0.045], **TIGHT)
    assert direct._last_momentum_solver is direct._fdm_u and not direct._by_step and direct._fdm_u.iterations == 0
    assert_close(direct, twin, "DoTimeStep and Advance mixed, " + scheme)


@pytest.mark.parametrize("scheme", ["euler", "cnab2"])
def test_the_switch_moves_between_calls(hip_engine, scheme):
    mixed, twin = fresh("2d", scheme, True, None, "fdm"), fresh("2d", scheme, True)
    tighten_statements(mixed)
    tighten_statements(twin)
    recs = [mixed.Advance(2, **TIGHT)]
    quiet(mixed.DoTimeStep)
    held = mixed._fdm_u
    mixed.SetImplicitSolve("cg")
    recs.append(mixed.Advance(1, **TIGHT))
    quiet(mixed.DoTimeStep)
    mixed.SetImplicitSolve("fdm")
    recs.append(mixed.Advance(1, **TIGHT))
    twin.Advance(2, **TIGHT)
    quiet(twin.DoTimeStep)
    twin.Advance(1, **TIGHT)
    quiet(twin.DoTimeStep)
    twin.Advance(1, **TIGHT)
    assert [r.implicit for r in recs] == ["fdm", "cg", "fdm"] and mixed._fdm_u is held and len(mixed._steppers) == 2
    assert (recs[1].mstar_iterations > 0).all() and (recs[2].mstar_iterations == 0).all()
    assert (recs[1].scalar_iterations > 0).all() and (recs[2].scalar_iterations == 0).all()
    assert_close(mixed, twin, "fdm, cg, fdm: " + scheme)


@pytest.mark.parametrize("scheme", ["euler", "cnab2"])
def test_an_object_back_at_cg_keeps_the_default_bits(hip_engine, scheme):
    """`SetImplicitSolve("fdm")` then `("cg")` before any step: the bits of an untouched object in `DoTimeStep`,
    `DoTimeStep(timestep=)` and `Advance`, fixed and variable."""
    def run(switch):
        ns = fresh("2d", scheme, True)
        if switch:
            ns.SetImplicitSolve("fdm")
            ns.SetImplicitSolve("cg")
        quiet(ns.DoTimeStep)
        quiet(ns.DoTimeStep, 0.03)
        recs = [ns.Advance(2), ns.Advance(2, timesteps=SIZES[:2])]
        assert all(r.implicit == "cg" for r in recs) and set(ns._steppers) == {"jacobi", ("variable", "jacobi")}
        return state(ns) + [r.mstar_iterations for r in recs] + [r.scalar_iterations for r in recs] \
            + [r.kinetic_energy for r in recs]
    for a, b in zip(run(False), run(True)):
        assert np.array_equal(a, b)


def test_set_implicit_solve_raises_for_a_system_that_does_not_factor(hip_engine):
    from templates.NavierStokesSIMPLE_iterative import NavierStokes, SyntheticMesh
    ns = NavierStokes(SyntheticMesh(0.25, dim=2), nu=0.01, inflow="inlet", outflow="outlet", wall="wall|cyl", uin=None,
                      timestep=TAU, order=1)
    assert ns.system.block_size > 1
    with pytest.raises(ValueError, match="SetImplicitSolve"):
        ns.SetImplicitSolve("fdm")
    assert ns.implicit_solve == "cg" and ns._fdm_u is None
