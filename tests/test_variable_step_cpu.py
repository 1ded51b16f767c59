"""Variable time steps on the CPU checker engine (no GPU): the order of the variable-step CN-AB2 scheme on its numpy
restatement (tests/variable_step_reference.py), the host controller `hipla.stepping.choose_timestep`, the controller on
the reference, and the product's statement path -- `DoTimeStep(timestep=)` stage by stage against the reference,
`Advance(cfl=)` / `Advance(timesteps=)` by statements, the defaults' bits, the errors, the exported symbols.

Tolerances: those of tests/test_cnab2_cpu.py (1e-13 in front of a solve, 1e-9 behind the velocity solve, 1e-8 behind
both converged inner solves)."""

import os
import re

import numpy as np
import pytest

from cnab2_reference import Cnab2Reference, smooth_start
from conftest import ROOT
from test_cnab2_cpu import (GRIDS, SCALARS, add_scalar, check_stages, fresh, mean_free, ratios, rel, scalar_args, step,
                            tighten)
from variable_step_reference import VariableStepReference

CODES = ("max", "cfl", "growth", "end")


# ---- 1. the order of the scheme under a variable step (reference only) -------------------------------------------------
@pytest.fixture(scope="module")
def cavity_16_fine():
    """The experiment of test_cnab2_cpu.py::test_reference_order_velocity (van Leer) with its fine run."""
    from staggered_grid import mac_stokes
    s = mac_stokes(2, 16, 0.01)
    u0, f = smooth_start(s), np.zeros(s.n_u)
    return s, u0, f, Cnab2Reference(s, 0.2 / 1280, u0, f, "vanleer").run(1280)


@pytest.mark.parametrize("pattern", [(1.5, 0.5), (1.0, 2.0, 0.5)])
def test_reference_order_under_a_variable_step(cavity_16_fine, pattern):
    """2-D n = 16, van Leer, end time 0.2, 12 / 24 / 48 / 96 steps whose sizes repeat `pattern` (scaled to mean 1).
    Velocity error ratios per halving, measured: (1.5, 0.5): 4.17 3.87 4.18 with the weights (1 + r/2, -r/2) and
    2.14 2.06 2.04 with (3/2, -1/2); (1, 2, 0.5): 4.32 4.16 4.18 and 2.08 2.02 2.01."""
    s, u0, f, fine = cavity_16_fine
    shape = np.array(pattern) / np.mean(pattern)
    errs = {}
    for naive in (False, True):
        errs[naive] = []
        for n in (12, 24, 48, 96):
            run = VariableStepReference(s, 0.2 / n, u0, f, "vanleer", naive=naive).run_pattern(0.2 / n, shape, n)
            errs[naive].append(rel(run.u, fine.u))
    print(pattern, errs, ratios(errs[False]), ratios(errs[True]))
    assert min(ratios(errs[False])) >= 3.5, ratios(errs[False])
    assert max(ratios(errs[True])) < 2.3, ratios(errs[True])


def test_reference_with_equal_steps_is_the_fixed_step_reference():
    """`step_with(tau)` with one size throughout has the bits of `Cnab2Reference.step` (r == 1 gives (3/2, -1/2))."""
    from staggered_grid import mac_stokes
    s = mac_stokes(2, 6, 0.01)
    u0, f = smooth_start(s), np.zeros(s.n_u)
    for scheme in ("euler", "cnab2"):
        a, b = Cnab2Reference(s, 0.03, u0, f, "minmod", scheme), VariableStepReference(s, 0.5, u0, f, "minmod", scheme)
        for _ in range(3):
            a.step()
            b.step_with(0.03)
        assert np.array_equal(a.u, b.u) and np.array_equal(a.q, b.q)


# ---- 2. choose_timestep ------------------------------------------------------------------------------------------------
def test_choose_timestep():
    from hipla.stepping import choose_timestep
    assert choose_timestep(2.0, 0.4, 0.05) == (0.05, "max")
    assert choose_timestep(16.0, 0.4, 0.05) == (0.4 / 16.0, "cfl")
    assert choose_timestep(16.0, 0.4, 0.05, previous=0.01) == (0.0125, "growth")
    assert choose_timestep(16.0, 0.4, 0.05, previous=0.01, growth=1.1) == (1.1 * 0.01, "growth")
    assert choose_timestep(16.0, 0.4, 0.05, previous=0.04) == (0.025, "cfl")
    # ties: "max" before "cfl" before "growth"
    assert choose_timestep(8.0, 0.4, 0.05) == (0.05, "max")
    assert choose_timestep(8.0, 0.4, 0.05, previous=0.04, growth=1.25) == (0.05, "max")
    assert choose_timestep(16.0, 0.4, 0.05, previous=0.02, growth=1.25) == (0.025, "cfl")
    assert choose_timestep(1.0, 0.4, 0.5, previous=0.25, growth=2.0) == (0.4, "cfl")
    # rate == 0: no CFL term
    assert choose_timestep(0.0, 0.4, 0.05) == (0.05, "max")
    assert choose_timestep(0.0, 0.4, 0.05, previous=0.01) == (0.0125, "growth")
    # remaining
    assert choose_timestep(2.0, 0.4, 0.05, remaining=0.2) == (0.05, "max")
    assert choose_timestep(2.0, 0.4, 0.05, remaining=0.03) == (0.03, "end")
    assert choose_timestep(2.0, 0.4, 0.05, remaining=0.05) == (0.05, "end")
    assert choose_timestep(2.0, 0.4, 0.05, remaining=0.05 * (1 + 5e-13)) == (0.05 * (1 + 5e-13), "end")
    assert choose_timestep(2.0, 0.4, 0.05, remaining=0.05 * (1 + 1e-11)) == (0.05, "max")
    assert choose_timestep(16.0, 0.4, 0.05, previous=0.01, remaining=0.012) == (0.012, "end")
    for bad in (float("nan"), float("inf"), -float("inf")):
        with pytest.raises(FloatingPointError):
            choose_timestep(bad, 0.4, 0.05)


# ---- 3. the controller on the reference --------------------------------------------------------------------------------
CONTROLLED = ("vanleer", "cnab2")       # the scheme that shows the measured codes: "cfl" x 4, then "max", at growth 1.25
#                                         (with "upwind" the third step is a near tie of "cfl" and "growth": 1.25000)


def controller_case():
    """2-D n = 8, nu = 0.05, smooth start with max |u| = 1: (system, u0, f)."""
    from staggered_grid import mac_stokes
    s = mac_stokes(2, 8, 0.05)
    return s, smooth_start(s, peak=1.0), np.zeros(s.n_u)


@pytest.fixture(scope="module")
def controlled_reference():
    """The two controlled runs of the reference, computed once: growth -> (sizes, codes, cfl numbers), and rate(u^0)."""
    s, u0, f = controller_case()
    runs = {}
    for growth, nsteps in ((1.25, 24), (1.1, 16)):
        ref = VariableStepReference(s, 0.05, u0, f, *CONTROLLED)
        runs[growth] = ref.run_controlled(nsteps, cfl=0.4, max_timestep=0.05, growth=growth)
    return runs, VariableStepReference(s, 0.05, u0, f).rate()


def test_controller_on_the_reference(controlled_reference):
    """cfl = 0.4, max_timestep = 0.05.  Measured: growth 1.25 over 24 steps: "cfl" x 4, then "max" x 20; growth 1.1 over
    16 steps: "cfl" x 1, "growth" x 7, "max" x 8."""
    runs, rate0 = controlled_reference
    assert abs(rate0 - 16.0) <= 16 * 1e-14, rate0
    counts = {code: sum(codes.count(code) for _, codes, _ in runs.values()) for code in ("max", "cfl", "growth")}
    print({g: codes for g, (_, codes, _) in runs.items()}, counts)
    assert all(count >= 3 for count in counts.values()), counts
    for taus, codes, numbers in runs.values():
        assert (numbers <= 0.4 * (1 + 1e-12)).all(), numbers
        assert codes[0] == "cfl" and abs(taus[0] - 0.4 / rate0) <= 1e-15
        assert (taus <= 0.05).all() and (taus > 0).all()


# ---- 4. the product on the numpy engine --------------------------------------------------------------------------------
def variable_reference_of(ns, grid, scalar):
    """The variable-step reference started from the state of `ns` (history and the size of its last step included)."""
    sc = None if SCALARS[scalar] is None else dict(scalar_args(grid, scalar), convection=ns._scalar.convection)
    ref = VariableStepReference(ns.system, ns.timestep, ns.gfu.numpy(), ns.f.vec.numpy(), ns.convection, ns.time_scheme,
                                scalar=sc, T0=None if sc is None else ns.temperature.numpy(), q0=ns.gfup.numpy())
    hist = ns._history
    if hist is not None and hist.valid["momentum"]:
        ref.F_prev, ref.valid["momentum"] = ns.F_prev.numpy().copy(), True
    if hist is not None and sc is not None and hist.valid["scalar"]:
        ref.G_prev, ref.valid["scalar"] = ns.G_prev.numpy().copy(), True
        ref.b_prev = None if ns.b_prev is None else ns.b_prev.numpy().copy()
    ref.tau_prev = ns._clock.tau_prev
    return ref


def step_with(ns, tau):
    import contextlib
    import io
    with contextlib.redirect_stdout(io.StringIO()):
        ns.DoTimeStep(timestep=tau)


def check_state(ns, want, scalar, tight):
    """What an "euler" step leaves to look at (it keeps no stages): u, the potential phi in gfup, and the scalar's
    temp_T, delta and T -- at the bounds of `check_stages`."""
    errs = dict(u=rel(ns.gfu.numpy(), want["u"]), q=rel(mean_free(ns.gfup.numpy()), mean_free(want["q"])))
    if SCALARS[scalar] is not None:
        errs.update(T=rel(ns.temperature.numpy(), want["T"]), temp_T=rel(ns._scalar.temp.numpy(), want["temp_T"]),
                    delta=rel(ns._scalar.delta.numpy(), want["delta"]))
    for key, err in errs.items():
        bound = 1e-8 if not tight or key in ("u", "q", "T") else 1e-9 if key == "delta" else 1e-13
        assert err < bound, (key, err, bound, errs)
    return errs


SIZES = (0.05, 0.03, 0.04, 0.02)       # the object's own size first; r = 0.6, 4/3, 1/2


@pytest.mark.parametrize("scalar", ["plain", "buoyant"])
@pytest.mark.parametrize("scheme", ["euler", "cnab2"])
@pytest.mark.parametrize("grid", list(GRIDS))
def test_do_time_step_with_a_size_against_the_reference(numpy_engine, grid, scheme, scalar):
    """Four `DoTimeStep(timestep=)` of four sizes on 2-D n = 8 and 3-D n = 5.  Every step against the reference run beside it from the common start (1e-8) and against one reference
    step started from the product's own state, history and last step size, stage by stage at the tight bounds."""
    ns = fresh_on(grid, "vanleer", scalar, scheme)
    beside = variable_reference_of(ns, grid, scalar)
    check = check_stages if scheme == "cnab2" else check_state
    for k, tau in enumerate(SIZES):
        own = variable_reference_of(ns, grid, scalar)
        assert own.tau_prev == (None if k == 0 else SIZES[k - 1])
        step_with(ns, tau)
        check(ns, beside.step_with(tau), scalar, tight=False)
        errs = check(ns, own.step_with(tau), scalar, tight=True)
        if scheme == "cnab2" and k:
            r = tau / SIZES[k - 1]
            assert own.weights("momentum") == (1 + r / 2, -r / 2)
            assert rel(ns.F_prev.numpy(), own.F_prev) < 1e-13
        assert ns._clock.tau_prev == tau
    print(grid, scheme, scalar, errs)
    assert len(ns._by_step) == 3 and 0.05 not in ns._by_step          # the object's own size runs its own operators


SIZES_OF = {"2d": 8, "3d": 5}


def fresh_on(grid, convection, scalar, scheme, **kw):
    """`fresh` of test_cnab2_cpu.py on 2-D n = 8 / 3-D n = 5."""
    import hipla
    from oracle import krylov_ref as kr
    from templates.NavierStokesSIMPLE_iterative import NavierStokes, SyntheticMesh
    dim, _, _ = GRIDS[grid]
    n = SIZES_OF[grid]
    ns = NavierStokes(SyntheticMesh(1.0 / n, dim=dim), nu=0.01, inflow="inlet", outflow="outlet", wall="wall|cyl",
                      uin=None, timestep=0.05, order=0, convection=convection, time_scheme=scheme, **kw)
    s = ns.system
    assert s.block_size == 1 and s.n == n
    ns.f.vec.data = hipla.Vector.from_numpy(0.1 * np.random.default_rng(8).standard_normal(s.n_u))
    u0 = 0.2 * kr.project(s.B, np.full(s.n_u, s.h ** s.dim), np.random.default_rng(2).standard_normal(s.n_u))[0]
    ns.gfu.data = hipla.Vector.from_numpy(u0)
    p0 = np.random.default_rng(4).standard_normal(s.n_p)
    ns.gfup.data = hipla.Vector.from_numpy(0.01 * (p0 - p0.mean()))
    add_scalar(ns, grid, scalar)
    return tighten(ns)


def controlled_product(scheme=CONTROLLED[1]):
    """The product on the controller case, converged inner solvers."""
    import hipla
    from templates.NavierStokesSIMPLE_iterative import NavierStokes, SyntheticMesh
    s, u0, f = controller_case()
    ns = NavierStokes(SyntheticMesh(1.0 / 8, dim=2), nu=0.05, inflow="inlet", outflow="outlet", wall="wall|cyl", uin=None,
                      timestep=0.05, order=0, convection=CONTROLLED[0], time_scheme=scheme)
    ns.f.vec.data = hipla.Vector.from_numpy(f)
    ns.gfu.data = hipla.Vector.from_numpy(u0)
    return tighten(ns)


@pytest.mark.parametrize("growth,nsteps", [(1.25, 24), (1.1, 16)])
def test_advance_with_cfl_by_statements(numpy_engine, controlled_reference, growth, nsteps):
    """`Advance(cfl=)` on the checker engine runs the controller through `DoTimeStep(timestep=tau_n)`: the reference's
    step sizes to 1e-9 relative, its codes exactly, every cfl[k] within the target."""
    taus, codes, numbers = controlled_reference[0][growth]
    ns = controlled_product()
    assert abs(ns.CflRate() - 16.0) <= 16 * 1e-14
    rec = ns.Advance(nsteps, precision=1e-14, maxsteps=(5000, 20000), cfl=0.4, growth=growth)
    assert rec.declined == "not the HIP engine" and rec.limited_by == codes
    assert np.abs(rec.timestep - taus).max() <= 1e-9 * taus.max() and (np.abs(rec.timestep / taus - 1) <= 1e-9).all()
    assert (rec.cfl <= 0.4 * (1 + 1e-12)).all() and np.allclose(rec.cfl, numbers, rtol=1e-8)
    assert np.array_equal(rec.time, np.cumsum(rec.timestep)) and len(rec.mstar_iterations) == nsteps
    assert ns._clock.tau_prev == rec.timestep[-1]


def test_duration_lands_on_the_end_time(numpy_engine):
    s, u0, f = controller_case()
    want = VariableStepReference(s, 0.05, u0, f, *CONTROLLED).run_controlled(40, 0.4, 0.05, duration=0.33)
    ns = controlled_product()
    rec = ns.Advance(40, precision=1e-14, maxsteps=(5000, 20000), cfl=0.4, duration=0.33)
    assert rec.limited_by[-1] == "end" and rec.limited_by.count("end") == 1 and rec.limited_by == want[1]
    assert abs(rec.time[-1] - 0.33) <= 1e-14 * 0.33 and len(rec.timestep) == len(want[0]) < 40
    assert 0 < rec.timestep[-1] <= 0.05 and (np.abs(rec.timestep / want[0] - 1) <= 1e-9).all()
    capped = controlled_product().Advance(3, cfl=0.4, duration=0.33)           # nsteps remains the cap
    assert len(capped.timestep) == 3 and "end" not in capped.limited_by


def test_prescribed_steps_by_statements(numpy_engine):
    """`Advance(timesteps=)` on the checker engine is `DoTimeStep(timestep=)` step by step, bit for bit, and records the
    sizes, the time and the CFL numbers; it mixes with fixed calls through the history."""
    a, b = fresh("2d", "vanleer", "buoyant"), fresh("2d", "vanleer", "buoyant")
    rates = []
    for tau in (0.05, 0.03, 0.04):
        rates.append(b.CflRate())
        step_with(b, tau)
    step(b)
    rec = a.Advance(3, timesteps=[0.05, 0.03, 0.04])
    a.Advance(1)
    assert np.array_equal(a.gfu.numpy(), b.gfu.numpy()) and np.array_equal(a.temperature.numpy(), b.temperature.numpy())
    assert np.array_equal(rec.timestep, [0.05, 0.03, 0.04]) and rec.limited_by is None
    assert np.array_equal(rec.time, np.cumsum([0.05, 0.03, 0.04])) and np.array_equal(rec.cfl, np.array(rates) * rec.timestep)
    assert (rec.scalar_iterations > 0).all() and (rec.mstar_iterations > 0).all()


# ---- 5. the defaults keep their bits -----------------------------------------------------------------------------------
def test_weights_and_tau_prev():
    from hipla.stepping import TimeHistory
    h = TimeHistory()
    assert h.tau_prev is None and h.weights("momentum") == h.weights("momentum", 0.03) == (1.0, 0.0)
    h.valid["momentum"], h.tau_prev = True, 0.05
    assert h.weights("momentum") == h.weights("momentum", 0.05) == (1.5, -0.5)       # r == 1.0: exactly
    assert h.weights("momentum", 0.03) == (1 + (0.03 / 0.05) / 2, -(0.03 / 0.05) / 2)
    assert h.weights("scalar", 0.03) == (1.0, 0.0)
    h.reset("scalar")
    assert h.tau_prev == 0.05
    h.reset()
    assert h.tau_prev is None and h.weights("momentum", 0.03) == (1.0, 0.0)


@pytest.mark.parametrize("scheme", ["euler", "cnab2"])
def test_plain_calls_keep_their_bits_and_record_the_step_size(numpy_engine, scheme):
    """`DoTimeStep()` equals `DoTimeStep(timestep=<the object's>)` bit for bit; `Advance(n)` has no variable-step
    fields; both record tau_prev = timestep; after `DoTimeStep(timestep=t)` a plain `DoTimeStep()` uses
    r = timestep / t; `ResetTimeHistory` clears tau_prev."""
    a, b = fresh("2d", "minmod", "buoyant", scheme), fresh("2d", "minmod", "buoyant", scheme)
    for _ in range(3):
        step(a)
        step_with(b, 0.05)
    assert np.array_equal(a.gfu.numpy(), b.gfu.numpy()) and np.array_equal(a.gfup.numpy(), b.gfup.numpy())
    assert np.array_equal(a.temperature.numpy(), b.temperature.numpy())
    assert a._clock.tau_prev == b._clock.tau_prev == 0.05 and not a._by_step and not b._by_step
    rec = a.Advance(2)
    assert rec.timestep is None and rec.time is None and rec.cfl is None and rec.limited_by is None
    assert a._clock.tau_prev == 0.05
    step_with(a, 0.02)
    assert a._clock.tau_prev == 0.02
    if scheme == "cnab2":
        assert a._history is a._clock
        assert a._history.weights("momentum", a.timestep) == (1 + (0.05 / 0.02) / 2, -(0.05 / 0.02) / 2)
        own = variable_reference_of(a, "2d", "buoyant")
        step(a)
        check_stages(a, own.step_with(0.05), "buoyant", tight=True)
        assert own.r == 0.05 / 0.02
    else:
        assert a._history is None
        step(a)
    assert a._clock.tau_prev == 0.05
    a.ResetTimeHistory()
    assert a._clock.tau_prev is None


# ---- 6. errors, the record, the symbols --------------------------------------------------------------------------------
def test_bad_arguments_raise(numpy_engine):
    ns = fresh("2d")
    u0 = ns.gfu.numpy().copy()
    bad = [dict(timesteps=[0.01, 0.02], cfl=0.4),
           dict(timesteps=[0.01, 0.02], inner_pre="amg"), dict(cfl=0.4, inner_pre="amg"),
           dict(timesteps=[0.01, 0.02], pseudo=True), dict(cfl=0.4, pseudo=True),
           dict(timesteps=[0.01, 0.0]), dict(timesteps=[0.01, -0.02]), dict(timesteps=[0.01, float("inf")]),
           dict(timesteps=[0.01, float("nan")]), dict(cfl=0.4, max_timestep=0.0), dict(cfl=0.4, max_timestep=float("nan")),
           dict(timesteps=[0.01]), dict(timesteps=[0.01, 0.02, 0.03]),
           dict(duration=0.1), dict(growth=1.5), dict(max_timestep=0.01),
           dict(timesteps=[0.01, 0.02], duration=0.1), dict(timesteps=[0.01, 0.02], growth=1.5),
           dict(timesteps=[0.01, 0.02], max_timestep=0.01),
           dict(cfl=0.4, growth=0.9)]
    for kw in bad:
        with pytest.raises(ValueError):
            ns.Advance(2, **kw)
    for t in (0.0, -0.01, float("inf"), float("nan")):
        with pytest.raises(ValueError):
            ns.DoTimeStep(timestep=t)
    assert np.array_equal(ns.gfu.numpy(), u0) and ns._clock.tau_prev is None


def test_non_finite_rate_raises(numpy_engine):
    import hipla
    ns = controlled_product()
    u = ns.gfu.numpy().copy()
    u[3] = np.nan
    ns.gfu.data = hipla.Vector.from_numpy(u)
    assert ns.CflRate() == np.inf
    with pytest.raises(FloatingPointError):
        ns.Advance(2, cfl=0.4)
    assert np.array_equal(ns.gfu.numpy(), u, equal_nan=True)


def test_symbols_are_declared_and_exported():
    import ctypes
    import __graft_entry__ as entry
    from hipla import fused
    from hipla.hip_engine import LIB_PATH, _signatures, load_library
    if not os.path.exists(LIB_PATH):
        entry.build()
    lib = load_library()
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "nss_krylov.h")).read(), flags=re.S)
    sigs = _signatures()
    for name in ("nss_cg_shift_jacobi_f64", "nss_step_cfl_f64", "nss_step_cfl_workspace"):
        assert hasattr(lib, name) and name in sigs and re.search(r"NSS_API\s+int\s+%s\s*\(" % name, text), name
        assert ctypes.c_void_p in sigs[name][1] or any("LP_" in t.__name__ for t in sigs[name][1]), name
    fields = [f for f, _ in fused.CgState._fields_]
    assert fields[-3:] == ["shift_mass", "shift_m0", "shift_sigma"]
    for field in ("shift_mass", "shift_m0", "shift_sigma"):
        assert re.search(r"\b%s\b" % field, text), field
    import hipla.stepping as st
    assert callable(st.choose_timestep) and callable(st.CflRate)
