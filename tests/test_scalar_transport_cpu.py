"""Scalar transport without a GPU: the grid operators of `StokesSystem.scalar_operators` (the exact discrete steady
state, conservation, the signs against B, the buoyancy force, the wall flux) and `NavierStokes.AddScalar` on the CPU
checker engine, where `Advance` declines and the statements of `DoTimeStep` run, against tests/scalar_reference.py.
Tolerances: DESIGN.md section 3 -- 1e-13 for an operator against numpy, 1e-9 / 1e-8 behind converged inner solves."""

import contextlib
import io

import numpy as np
import pytest

from scalar_reference import coupled_step

WALLS = {"x-": 1.0, "x+": 0.0}


def rel(a, b):
    return np.linalg.norm(a - b) / np.linalg.norm(b)


def cell_x(s):
    """x of the cell centres (x is the fastest index)."""
    return np.tile((np.arange(s.n) + 0.5) * s.h, s.n ** (s.dim - 1))


@pytest.mark.parametrize("dim,n", [(2, 6), (3, 4)])
def test_linear_profile_is_the_discrete_steady_state(dim, n):
    from staggered_grid import mac_stokes
    s = mac_stokes(dim, n, 0.01)
    ops = s.scalar_operators(0.37, WALLS)
    T = 1.0 - cell_x(s)
    assert np.abs(ops["K"] @ T - ops["q"]).max() <= 1e-13 * np.abs(ops["q"]).max()
    assert abs(ops["K"] - ops["K"].T).max() == 0.0
    assert ops["mass"] is s.mass
    for key in ("avg", "diff"):
        assert ops[key].shape == (s.n_u, s.n_p) and (np.diff(ops[key].indptr) == 2).all()
    assert np.array_equal(ops["avg"].indices, ops["diff"].indices)       # avg and diff share their columns


@pytest.mark.parametrize("dim,n", [(2, 6), (3, 4)])
def test_insulated_box_conserves_the_scalar(dim, n):
    from staggered_grid import mac_stokes
    s = mac_stokes(dim, n, 0.01)
    ops = s.scalar_operators(1.0, {})
    rng = np.random.default_rng(3)
    u, T = rng.standard_normal(s.n_u), rng.standard_normal(s.n_p)
    G = u * (ops["avg"] @ T) - 0.5 * np.abs(u) * (ops["diff"] @ T)
    terms = np.abs(s.B) @ np.abs(G)
    assert abs(np.ones(s.n_p) @ (s.B @ G)) <= 1e-14 * terms.sum()
    assert not ops["q"].any() and np.abs(ops["K"] @ np.ones(s.n_p)).max() <= 1e-14 * ops["K"].diagonal().max()


@pytest.mark.parametrize("dim,n", [(2, 5), (3, 4)])
def test_flux_divergence_against_direct_loops(dim, n):
    """-B G against `scalar_convection_reference`: the signs of avg and diff against B, for u of both signs."""
    from staggered_grid import mac_stokes
    s = mac_stokes(dim, n, 0.01)
    ops = s.scalar_operators(1.0, WALLS)
    rng = np.random.default_rng(4)
    u, T = rng.standard_normal(s.n_u), rng.standard_normal(s.n_p)
    assert (u > 0).any() and (u < 0).any()
    G = u * (ops["avg"] @ T) - 0.5 * np.abs(u) * (ops["diff"] @ T)
    want = s.scalar_convection_reference(u, T)
    scale = np.abs(s.B) @ (np.abs(u) * (np.abs(ops["avg"]) @ np.abs(T)) + 0.5 * np.abs(u) * (np.abs(ops["diff"]) @ np.abs(T)))
    assert (np.abs(-(s.B @ G) - want) <= 2e-16 * scale.max()).all()
    central = -(s.B @ (u * (ops["avg"] @ T)))
    assert np.linalg.norm(central - want) > 1e-3 * np.linalg.norm(want)      # the upwind term is there


def test_uniform_reference_temperature_gives_no_force():
    from staggered_grid import mac_stokes
    s = mac_stokes(2, 6, 0.01)
    ops = s.scalar_operators(1.0, WALLS)
    w_b = s.buoyancy_weights((0.3, 710.0))
    assert np.count_nonzero(w_b) == s.n_u and set(np.unique(w_b)) == {0.3 * s.h ** 2, 710.0 * s.h ** 2}
    assert (w_b[s.component_ids[1].ravel()] == 710.0 * s.h ** 2).all()
    f = np.random.default_rng(5).standard_normal(s.n_u)
    t_ref = 0.3
    assert np.array_equal(f + w_b * (ops["avg"] @ np.full(s.n_p, t_ref) - t_ref), f)
    with pytest.raises(ValueError):
        s.buoyancy_weights((1.0,))


def test_wall_flux_of_the_linear_profile():
    from staggered_grid import mac_stokes
    s = mac_stokes(2, 6, 0.01)
    kappa = 0.37
    ops = s.scalar_operators(kappa, WALLS)
    T = 1.0 - cell_x(s)
    c0, w = ops["wall_flux"]("x-")
    assert abs((c0 - w @ T) - kappa) <= 1e-13 * kappa
    c0, w = ops["wall_flux"]("x+")
    assert abs((c0 - w @ T) + kappa) <= 1e-13 * kappa               # what enters on the left leaves on the right
    with pytest.raises(ValueError):
        ops["wall_flux"]("y-")
    with pytest.raises(ValueError):
        s.scalar_operators(1.0, {"z-": 1.0})
    with pytest.raises(ValueError):
        s.inflate(2).scalar_operators(1.0, WALLS)


# ---- NavierStokes.AddScalar on the checker engine -----------------------------------------------------------------
SCALAR = dict(kappa=0.8, dirichlet=WALLS, buoyancy=(0.0, 40.0), t_ref=0.5)


def fresh(dim, **scalar):
    import hipla
    from templates.NavierStokesSIMPLE_iterative import NavierStokes, SyntheticMesh
    ns = NavierStokes(SyntheticMesh(0.2 if dim == 2 else 0.25, dim=dim), nu=0.01, inflow="inlet", outflow="outlet",
                      wall="wall|cyl", uin=None, timestep=0.05, order=0)
    s = ns.system
    assert s.block_size == 1
    ns.AddForce(0.1 * np.random.default_rng(8).standard_normal(s.n_u))
    ns.gfu.data = hipla.Vector.from_numpy(0.1 * np.random.default_rng(2).standard_normal(s.n_u))
    if scalar:
        ns.AddScalar(initial=np.random.default_rng(6).random(s.n_p), precision=1e-14, maxsteps=5000, **scalar)
    ops = ns._time_stepping_operators()
    ops["invmstar"] = hipla.CGSolver(ops["mstar"], pre=hipla.JacobiPreconditioner(ops["mstar"]), precision=1e-14, maxsteps=5000)
    ops["invproj"] = hipla.CGSolver(ops["Lp"], pre=hipla.JacobiPreconditioner(ops["Lp"]), precision=1e-14, maxsteps=20000)
    return ns


@pytest.mark.parametrize("dim", [2, 3])
@pytest.mark.parametrize("buoyant", [True, False])
def test_statements_against_the_reference(numpy_engine, dim, buoyant):
    """Three `DoTimeStep` calls and `Advance(3)` (declined: the same statements) against `coupled_step` step by step:
    the increment delta to 1e-9, T and u to 1e-8, the recorded wall flux to 1e-8."""
    scalar = dict(SCALAR, buoyancy=((0.0, 40.0) if dim == 2 else (0.0, 40.0, -3.0)) if buoyant else None)
    ns, twin = fresh(dim, **scalar), fresh(dim, **scalar)
    s = ns.system
    u, T, f = ns.gfu.numpy(), ns.temperature.numpy(), ns.f.vec.numpy()
    walls = []
    for step in range(3):
        want = coupled_step(s, ns.timestep, u, T, f, **scalar)
        with contextlib.redirect_stdout(io.StringIO()):
            ns.DoTimeStep()
        assert rel(ns._scalar.G.numpy(), want["G"]) < 1e-13
        assert rel(ns._scalar.temp.numpy(), want["temp_T"]) < 1e-9       # (behind u^n, itself behind two solves)
        assert rel(ns._scalar.delta.numpy(), want["delta"]) < 1e-9
        assert rel(ns.temperature.numpy(), want["T"]) < 1e-8
        assert rel(ns.gfu.numpy(), want["u"]) < 1e-8
        if buoyant:
            assert rel(ns._scalar.f_eff.numpy(), want["f_eff"]) < 1e-9
            assert np.linalg.norm(want["f_eff"] - f) > 1e-3 * np.linalg.norm(f)
        else:
            assert np.array_equal(want["f_eff"], f)
        u, T = want["u"], want["T"]
        walls.append(want["wall_flux"])
    rec = twin.Advance(3, precision=1e-14, maxsteps=(5000, 20000))
    assert rec.declined == "not the HIP engine"
    assert np.array_equal(twin.temperature.numpy(), ns.temperature.numpy())
    assert np.array_equal(twin.gfu.numpy(), ns.gfu.numpy())
    assert rec.scalar_iterations.shape == (3,) and (rec.scalar_iterations > 0).all()
    assert np.abs(rec.wall_flux - np.array(walls)).max() <= 1e-8 * np.abs(walls).max()
    assert twin.Advance(1, diagnostics=False).wall_flux is None
    with pytest.raises(ValueError):
        twin.Advance(1, pseudo=True)


def test_advance_without_a_scalar_has_no_scalar_record(numpy_engine):
    ns = fresh(2)
    rec = ns.Advance(2)
    assert rec.scalar_iterations is None and rec.wall_flux is None
    assert not hasattr(ns, "temperature") and ns._scalar is None
    assert len(ns.Advance(1, pseudo=True).proj_iterations) == 1     # the pseudo time stepping still runs without one


def test_add_scalar_arguments(numpy_engine):
    from templates.NavierStokesSIMPLE_iterative import NavierStokes, SyntheticMesh
    ns = fresh(2)
    ns.AddScalar(1.0, dirichlet={"y+": 2.0, "x-": 1.0}, t_ref=0.25)
    assert np.array_equal(ns.temperature.numpy(), np.full(ns.system.n_p, 0.25))
    assert ns._scalar.flux_wall == "y+" and ns._scalar.Wb is None
    assert (ns._scalar.inv.precision, ns._scalar.inv.maxsteps) == (1e-4, 500)
    ns.AddScalar(1.0, dirichlet=WALLS, buoyancy=(0.3, 7.0), t_ref=0.25)     # T = t_ref everywhere: no force, exactly
    assert np.array_equal(ns._scalar_flux().numpy(), ns.f.vec.numpy()) and ns._scalar.Wb is not None
    ns.AddScalar(1.0)                                               # all walls insulated: nothing to record
    assert ns.Advance(1).wall_flux is None
    with pytest.raises(ValueError):
        ns.AddScalar(1.0, initial=np.zeros(3))
    inflated = NavierStokes(SyntheticMesh(0.2, dim=2), nu=0.01, inflow="inlet", outflow="outlet", wall="wall|cyl",
                            uin=None, timestep=0.05, order=1)
    with pytest.raises(ValueError):
        inflated.AddScalar(1.0, dirichlet=WALLS)
