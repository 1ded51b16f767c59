"""`NavierStokes(time_scheme="cnab2")` on the CPU checker engine (no GPU): the order of the scheme on its numpy
restatement (tests/cnab2_reference.py), the statements of `DoTimeStep` against that restatement stage by stage, and the
public surface -- the default path's bits, the history and its reset, the errors.

Tolerances (as in the existing time-stepper tests): 1e-13 for `temp` (no solve in front of it),
1e-9 for `raw`, 1e-8 for what lies behind both converged inner solves."""

import contextlib
import io

import numpy as np
import pytest

from cnab2_reference import Cnab2Reference, order_errors, smooth_start
from oracle import krylov_ref as kr

TAU = 0.05
WALLS = {"x-": 1.0, "x+": 0.0}
GRIDS = {"2d": (2, 5, (0.0, 2.0)), "3d": (3, 4, (0.0, 2.0, -1.0))}
SCALARS = {"plain": None, "passive": False, "buoyant": True}


def rel(a, b):
    return np.linalg.norm(np.asarray(a) - b) / np.linalg.norm(b)


def mean_free(p):
    """The pressure of the enclosed domain is fixed up to a constant (B^T 1 = 0; a Jacobi-CG iterate is not mean free)."""
    return p - p.mean()


def ratios(errs):
    return [errs[i] / errs[i + 1] for i in range(len(errs) - 1)]


# ---- 1. the order of the scheme (reference only) --------------------------------------------------------------------
@pytest.fixture(scope="module")
def cavity_16():
    from staggered_grid import mac_stokes
    s = mac_stokes(2, 16, 0.01)
    return s, smooth_start(s), np.zeros(s.n_u)


@pytest.mark.parametrize("convection", ["upwind", "vanleer"])
def test_reference_order_velocity(cavity_16, convection):
    """2-D n = 16, nu = 0.01, T = 0.2, smooth start with max |u| = 1, errors against 1280 steps of "cnab2".  Measured
    (10 / 20 / 40 / 80 steps):
        upwind   euler  1.445e-02 7.399e-03 3.745e-03 1.884e-03   ratios 1.95 1.98 1.99
        upwind   cnab2  4.329e-04 1.066e-04 2.646e-05 6.576e-06   ratios 4.06 4.03 4.02
        van Leer euler  1.511e-02 7.712e-03 3.897e-03 1.959e-03   ratios 1.96 1.98 1.99
        van Leer cnab2  5.907e-04 1.444e-04 3.591e-05 8.896e-06   ratios 4.09 4.02 4.04
    i.e. "cnab2" is 220 to 290 times more accurate at 80 steps."""
    s, u0, f = cavity_16
    fine = Cnab2Reference(s, 0.2 / 1280, u0, f, convection).run(1280)
    assert np.linalg.norm(s.B @ fine.u) < 1e-12 * np.linalg.norm(fine.u) / s.h       # |B u| at rounding level
    errs = {scheme: [e for e, _ in order_errors(s, 0.2, (10, 20, 40, 80), fine, u0, f, convection, scheme)]
            for scheme in ("euler", "cnab2")}
    print(convection, errs, ratios(errs["euler"]), ratios(errs["cnab2"]))
    assert min(ratios(errs["cnab2"])) >= 3.5
    assert max(ratios(errs["euler"])) < 2.2
    assert errs["euler"][-1] >= 50 * errs["cnab2"][-1]


@pytest.mark.parametrize("convection", ["upwind", "vanleer"])
def test_product_runs_the_experiment_of_the_reference(numpy_engine, cavity_16, convection):
    """The 10-step run of the experiment above through `NavierStokes(time_scheme="cnab2").DoTimeStep` with converged
    inner solves lands on the reference's 10-step state to 1e-7 (ten steps of 1e-8 each), i.e. four digits inside the
    4e-4 the scheme itself errs by at that step size."""
    import hipla
    from templates.NavierStokesSIMPLE_iterative import NavierStokes, SyntheticMesh
    s, u0, f = cavity_16
    ns = NavierStokes(SyntheticMesh(1.0 / 16, dim=2), nu=0.01, inflow="inlet", outflow="outlet", wall="wall|cyl", uin=None,
                      timestep=0.02, order=0, convection=convection, time_scheme="cnab2")
    assert ns.system.n == 16 and ns.system.n_u == s.n_u
    ns.f.vec.data = hipla.Vector.from_numpy(f)
    ns.gfu.data = hipla.Vector.from_numpy(u0)
    tighten(ns)
    for _ in range(10):
        step(ns)
    want = Cnab2Reference(s, 0.02, u0, f, convection).run(10)
    assert rel(ns.gfu.numpy(), want.u) < 1e-7 and rel(mean_free(ns.gfup.numpy()), mean_free(want.q)) < 1e-7


def test_reference_order_coupled():
    """2-D n = 12, heated side walls, kappa = 0.02, buoyancy (0, 20), from rest to T = 1 (max |u| = 1.41), errors against
    1600 steps of "cnab2".  Measured (25 / 50 / 100 / 200 steps):
        euler u  4.038e-02 1.986e-02 9.859e-03 4.915e-03   ratios 2.03 2.01 2.01
        euler T  2.383e-02 1.127e-02 5.473e-03 2.696e-03   ratios 2.11 2.06 2.03
        cnab2 u  5.175e-03 1.259e-03 3.120e-04 7.698e-05   ratios 4.11 4.04 4.05
        cnab2 T  1.893e-03 4.638e-04 1.153e-04 2.850e-05   ratios 4.08 4.02 4.05"""
    from staggered_grid import mac_stokes
    s = mac_stokes(2, 12, 0.01)
    sc = dict(kappa=0.02, dirichlet=WALLS, buoyancy=(0.0, 20.0), t_ref=0.5)
    u0 = f = np.zeros(s.n_u)
    fine = Cnab2Reference(s, 1.0 / 1600, u0, f, "upwind", scalar=sc).run(1600)
    assert 1.3 < np.abs(fine.u).max() < 1.5 and np.linalg.norm(s.B @ fine.u) < 1e-12 * np.linalg.norm(fine.u) / s.h
    errs = {scheme: order_errors(s, 1.0, (25, 50, 100, 200), fine, u0, f, "upwind", scheme, scalar=sc)
            for scheme in ("euler", "cnab2")}
    for k, name in enumerate(("u", "T")):
        euler, cnab2 = ([pair[k] for pair in errs[scheme]] for scheme in ("euler", "cnab2"))
        print(name, euler, ratios(euler), cnab2, ratios(cnab2))
        assert min(ratios(cnab2)) >= 3.5, (name, ratios(cnab2))
        assert max(ratios(euler)) < 2.2, (name, ratios(euler))
        assert euler[-1] >= 50 * cnab2[-1], (name, euler[-1], cnab2[-1])


# ---- 2. DoTimeStep against the reference ----------------------------------------------------------------------------
def fresh(grid, convection="upwind", scalar="plain", time_scheme="cnab2", **kw):
    """A `NavierStokes` with converged inner solvers, a seeded divergence-free start (max |u| tau / h about 0.1), a
    seeded force and a seeded start pressure in gfup."""
    import hipla
    from templates.NavierStokesSIMPLE_iterative import NavierStokes, SyntheticMesh
    dim, n, beta = GRIDS[grid]
    extra = dict(kw) if time_scheme is None else dict(kw, time_scheme=time_scheme)
    ns = NavierStokes(SyntheticMesh(1.0 / n, dim=dim), nu=0.01, inflow="inlet", outflow="outlet", wall="wall|cyl",
                      uin=None, timestep=TAU, order=0, convection=convection, **extra)
    s = ns.system
    assert s.block_size == 1 and s.n == n
    ns.f.vec.data = hipla.Vector.from_numpy(0.1 * np.random.default_rng(8).standard_normal(s.n_u))
    u0 = 0.2 * kr.project(s.B, np.full(s.n_u, s.h ** s.dim), np.random.default_rng(2).standard_normal(s.n_u))[0]
    ns.gfu.data = hipla.Vector.from_numpy(u0)
    p0 = np.random.default_rng(4).standard_normal(s.n_p)
    ns.gfup.data = hipla.Vector.from_numpy(0.01 * (p0 - p0.mean()))
    add_scalar(ns, grid, scalar)
    return tighten(ns)


def scalar_args(grid, scalar):
    return dict(kappa=0.8, dirichlet=WALLS, buoyancy=GRIDS[grid][2] if SCALARS[scalar] else None, t_ref=0.5)


def add_scalar(ns, grid, scalar):
    if SCALARS[scalar] is not None:
        ns.AddScalar(initial=np.random.default_rng(6).random(ns.system.n_p), precision=1e-14, maxsteps=5000,
                     **scalar_args(grid, scalar))


def tighten(ns):
    """The inner solvers of the statements run to convergence."""
    import hipla
    ops = ns._time_stepping_operators()
    ops["invmstar"] = hipla.CGSolver(ops["mstar"], pre=hipla.JacobiPreconditioner(ops["mstar"]), precision=1e-14, maxsteps=5000)
    ops["invproj"] = hipla.CGSolver(ops["Lp"], pre=hipla.JacobiPreconditioner(ops["Lp"]), precision=1e-14, maxsteps=20000)
    if ns.time_scheme == "cnab2":
        half = ns._cnab2_operators()
        half["invmhalf"] = hipla.CGSolver(half["mhalf"], pre=hipla.JacobiPreconditioner(half["mhalf"]), precision=1e-14,
                                          maxsteps=5000)
    return ns


def reference_of(ns, grid, scalar):
    """The reference started from the state of `ns` (history included)."""
    sc = None if SCALARS[scalar] is None else dict(scalar_args(grid, scalar), convection=ns._scalar.convection)
    ref = Cnab2Reference(ns.system, ns.timestep, ns.gfu.numpy(), ns.f.vec.numpy(), ns.convection, ns.time_scheme,
                         scalar=sc, T0=None if sc is None else ns.temperature.numpy(), q0=ns.gfup.numpy())
    hist = ns._history
    if hist is not None and hist.valid["momentum"]:
        ref.F_prev, ref.valid["momentum"] = ns.F_prev.numpy().copy(), True
    if hist is not None and sc is not None and hist.valid["scalar"]:
        ref.G_prev, ref.valid["scalar"] = ns.G_prev.numpy().copy(), True
        ref.b_prev = None if ns.b_prev is None else ns.b_prev.numpy().copy()
    return ref


def step(ns):
    with contextlib.redirect_stdout(io.StringIO()):
        ns.DoTimeStep()


def check_stages(ns, want, scalar, tight):
    """The stages of the last `DoTimeStep` against `want`; `tight`: the step started from the reference's own state."""
    got = {k: v.numpy() for k, v in ns.last_stages.items()}
    errs = {k: rel(got[k], want[k]) for k in ("F_ext", "temp", "raw", "temp2")}
    errs.update(u=rel(ns.gfu.numpy(), want["u"]), q=rel(mean_free(ns.gfup.numpy()), mean_free(want["q"])))
    if SCALARS[scalar] is not None:
        errs.update(T=rel(ns.temperature.numpy(), want["T"]), G_ext=rel(ns._scalar.G_ext.numpy(), want["G_ext"]),
                    temp_T=rel(ns._scalar.temp.numpy(), want["temp_T"]), delta=rel(ns._scalar.delta.numpy(), want["delta"]))
    if SCALARS[scalar]:
        errs.update(f_step=rel(ns._scalar.f_eff.numpy(), want["f_step"]))
    for key, err in errs.items():
        bound = 1e-8 if not tight or key in ("temp2", "u", "q", "T") else 1e-9 if key in ("raw", "delta") else 1e-13
        assert err < bound, (key, err, bound, errs)
    return errs


@pytest.mark.parametrize("scalar", list(SCALARS))
@pytest.mark.parametrize("convection", ["upwind", "minmod", "vanleer"])
@pytest.mark.parametrize("grid", list(GRIDS))
def test_do_time_step_against_the_reference(numpy_engine, grid, convection, scalar):
    """Five `DoTimeStep`s.  Every step against the reference run beside it from the common start (1e-8: the solves'
    errors of the earlier steps are in the state); steps 1, 3 and 5 also against one reference step started from the
    product's own state and history, stage by stage at the tight bounds -- step 1 with the weights (1, 0), steps 3 and
    5 with (3/2, -1/2)."""
    ns = fresh(grid, convection, scalar)
    beside = reference_of(ns, grid, scalar)
    for k in range(1, 6):
        own = reference_of(ns, grid, scalar) if k in (1, 3, 5) else None
        assert own is None or own.weights("momentum") == ((1.0, 0.0) if k == 1 else (1.5, -0.5))
        step(ns)
        check_stages(ns, beside.step(), scalar, tight=False)
        if own is not None:
            errs = check_stages(ns, own.step(), scalar, tight=True)
            assert rel(ns.F_prev.numpy(), own.F_prev) < 1e-13
            assert SCALARS[scalar] is None or rel(ns.G_prev.numpy(), own.G_prev) < 1e-13
            assert not SCALARS[scalar] or rel(ns.b_prev.numpy(), own.b_prev) < 1e-13
    print(grid, convection, scalar, errs)
    s, u = ns.system, ns.gfu.numpy()
    assert np.linalg.norm(s.B @ u) < 1e-8 * np.linalg.norm(u) / s.h
    assert np.abs(u).max() * TAU / s.h < 0.5


def test_scalar_added_later_starts_with_first_step_weights(numpy_engine):
    """A scalar added after two steps extrapolates with (1, 0) while the momentum flux keeps (3/2, -1/2)."""
    ns = fresh("2d", "vanleer", "plain")
    step(ns)
    step(ns)
    add_scalar(ns, "2d", "buoyant")
    assert ns._history.weights("momentum") == (1.5, -0.5) and ns._history.weights("scalar") == (1.0, 0.0)
    own = reference_of(ns, "2d", "buoyant")
    assert own.valid == {"momentum": True, "scalar": False}
    for _ in range(2):
        step(ns)
        check_stages(ns, own.step(), "buoyant", tight=False)
    assert ns._history.weights("scalar") == (1.5, -0.5)


# ---- 3. the public surface ------------------------------------------------------------------------------------------
def test_euler_is_the_default_bit_for_bit(numpy_engine):
    """`time_scheme="euler"` and no keyword: identical bits over three steps with a buoyant scalar, no history, none of
    the operators of "cnab2"."""
    a, b = fresh("2d", "vanleer", "buoyant", time_scheme=None), fresh("2d", "vanleer", "buoyant", time_scheme="euler")
    for ns in (a, b):
        for _ in range(3):
            step(ns)
        assert ns.time_scheme == "euler"
        assert ns.F_prev is None and ns.G_prev is None and ns.b_prev is None and ns._history is None
        assert ns._stepping_cnab2 is None and ns.last_stages is None
        assert not hasattr(ns._scalar, "mhalf") and not hasattr(ns._scalar, "G_ext")
        ns.ResetTimeHistory()                                                      # nothing to forget
    assert np.array_equal(a.gfu.numpy(), b.gfu.numpy()) and np.array_equal(a.gfup.numpy(), b.gfup.numpy())
    assert np.array_equal(a.temperature.numpy(), b.temperature.numpy())
    rec = a.Advance(1)
    assert rec.time_scheme == "euler"


def test_bad_arguments_raise(numpy_engine):
    import hipla
    with pytest.raises(ValueError, match="time_scheme"):
        fresh("2d", time_scheme="rk4")

    class NoFlux(hipla.BaseMatrix):
        def __init__(self, n):
            super().__init__()
            self.n = n

        def Height(self):
            return self.n

        def Width(self):
            return self.n

        def Mult(self, x, y):
            y.data = 0.0 * x

    ns = fresh("2d")
    ns.conv_operator = NoFlux(ns.system.n_u)
    u0 = ns.gfu.numpy().copy()
    with pytest.raises(ValueError, match="Flux"):
        ns.DoTimeStep()
    assert np.array_equal(ns.gfu.numpy(), u0)
    euler = fresh("2d", time_scheme="euler")                 # the first-order step takes such an operator, as ever
    euler.conv_operator = NoFlux(euler.system.n_u)
    step(euler)


@pytest.mark.parametrize("scalar", ["plain", "buoyant"])
def test_reset_time_history(numpy_engine, scalar):
    """The step after `ResetTimeHistory()` equals, bit for bit, the first step of a fresh object started from the same
    state; without the reset it does not.  The accumulated pressure is left alone."""
    import hipla
    ns = fresh("2d", "minmod", scalar)
    step(ns)
    step(ns)
    state = [ns.gfu.numpy().copy(), ns.gfup.numpy().copy()] + ([ns.temperature.numpy().copy()] if SCALARS[scalar] else [])
    twin, kept = fresh("2d", "minmod", scalar), fresh("2d", "minmod", scalar)
    step(kept)
    step(kept)
    ns.ResetTimeHistory()
    assert np.array_equal(ns.gfup.numpy(), state[1])
    assert ns._history.weights("momentum") == ns._history.weights("scalar") == (1.0, 0.0)
    twin.gfu.data = hipla.Vector.from_numpy(state[0])
    twin.gfup.data = hipla.Vector.from_numpy(state[1])
    if SCALARS[scalar]:
        twin.temperature.data = hipla.Vector.from_numpy(state[2])
    for obj in (ns, twin, kept):
        step(obj)
    assert np.array_equal(ns.gfu.numpy(), twin.gfu.numpy()) and np.array_equal(ns.gfup.numpy(), twin.gfup.numpy())
    assert not SCALARS[scalar] or np.array_equal(ns.temperature.numpy(), twin.temperature.numpy())
    assert rel(ns.gfu.numpy(), kept.gfu.numpy()) > 1e-6


def test_advance_by_statements_follows_the_scheme(numpy_engine):
    """Not the HIP engine: `Advance` runs `DoTimeStep`, so `Advance(2)` + `DoTimeStep` equals three `DoTimeStep`s bit
    for bit, the record names the scheme and counts the half-step solver's iterations; `pseudo=True` stays the
    relaxation of the first-order operators and records "euler"."""
    ns, twin = fresh("2d", "vanleer", "buoyant"), fresh("2d", "vanleer", "buoyant")
    rec = ns.Advance(2, precision=1e-14, maxsteps=(5000, 20000))
    step(ns)
    for _ in range(3):
        step(twin)
    assert rec.declined == "not the HIP engine" and rec.time_scheme == "cnab2"
    assert (rec.mstar_iterations > 0).all() and (rec.scalar_iterations > 0).all()
    assert np.array_equal(ns.gfu.numpy(), twin.gfu.numpy()) and np.array_equal(ns.gfup.numpy(), twin.gfup.numpy())
    assert np.array_equal(ns.temperature.numpy(), twin.temperature.numpy())
    plain, relax = fresh("2d"), fresh("2d", time_scheme="euler")
    rec = plain.Advance(2, pseudo=True)
    relax.Advance(2, pseudo=True)
    assert rec.time_scheme == "euler" and np.array_equal(plain.gfu.numpy(), relax.gfu.numpy())
    assert plain._history.valid == {"momentum": False, "scalar": False}
