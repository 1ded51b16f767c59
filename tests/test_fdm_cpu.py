"""The fast diagonalisation of the pressure operator on the host (no GPU): `hipla.fdm_factors` on the grids of this
package, the numpy restatement of the solve against a Jacobi-CG run, the declines, and `NavierStokes.SetProjection` on
the CPU checker engine.

Bounds.  The comparison of the Kronecker sum with Lp: 1e-12 max |Lp| (the bound `fdm_factors` itself declines at; measured
2e-16).  The restatement: residual <= 1e-13 |rhs| (measured at most 2.5e-15 on these grids: a margin of 40 for other
BLAS summation orders), |mean phi| <= 1e-13 max |phi|.  C phi against Jacobi-CG run to 1e-13: 1e-10 |vel| (measured
2e-13; the CG's own error is its tolerance times the condition number).  The template: 1e-9 |u| against a twin whose CG
projection runs to 1e-13, both with the velocity solve at 1e-13 -- at its default 1e-4 the stopping iteration of that
solve is not a continuous function of its input, and the twins' inputs differ by the 1e-10 of the projections."""

import contextlib
import io

import numpy as np
import pytest
import scipy.sparse as sp

from oracle import krylov_ref as kr

CASES = {"2d_n2": (2, 2, 1), "2d_n5": (2, 5, 1), "2d_n12": (2, 12, 1), "3d_n2": (3, 2, 1), "3d_n4": (3, 4, 1),
         "3d_n7": (3, 7, 1), "3d_n5_inflated3": (3, 5, 3)}


def system_of(case):
    from staggered_grid import mac_stokes
    dim, n, bs = CASES[case]
    s = mac_stokes(dim, n, 0.01)
    return s.inflate(bs) if bs > 1 else s


def projection_operators(s):
    """(Lp, C) = (B M_u^-1 B^T, M_u^-1 B^T) with the template's lumped velocity mass h^dim."""
    C = (sp.diags(np.full(s.n_u, 1.0 / s.h ** s.dim)) @ s.B.T).tocsr()
    Lp = (s.B @ C).tocsr()
    Lp.sort_indices()
    return Lp, C


@pytest.fixture(scope="module", params=sorted(CASES))
def case(request):
    from hipla.fdm import fdm_factors
    s = system_of(request.param)
    Lp, C = projection_operators(s)
    factors, why = fdm_factors(Lp, (s.n,) * s.dim)
    assert why is None and factors is not None, why
    return s, Lp, C, factors


def jacobi_cg(A, b, tol, maxsteps=20000):
    """Jacobi-preconditioned CG from zero, stopped at sqrt <r, z> < tol * its first value: (x, iterations)."""
    dinv = 1.0 / A.diagonal()
    x, r = np.zeros_like(b), b.copy()
    z = dinv * r
    p, rz = z.copy(), r @ z
    err0 = np.sqrt(abs(rz))
    for it in range(maxsteps):
        q = A @ p
        alpha = rz / (p @ q)
        x += alpha * p
        r -= alpha * q
        z = dinv * r
        rz_new = r @ z
        if np.sqrt(abs(rz_new)) < tol * err0:
            return x, it + 1
        p = z + (rz_new / rz) * p
        rz = rz_new
    raise AssertionError("jacobi_cg did not converge")


# ---- 1. the factors ---------------------------------------------------------------------------------------------------
def test_kronecker_sum_equals_the_pressure_operator(case):
    s, Lp, _, factors = case
    K = factors.kronecker_sum()
    top = abs(Lp).max()
    err = abs(Lp - K).max() / top
    print("max |Lp - K| / max |Lp| = %.3g (reported %.3g)" % (err, factors.error))
    assert err <= 1e-12 and factors.error <= 1e-12
    assert factors.extents == (s.n,) * s.dim
    for t, q, lam in zip(factors.T, factors.Q, factors.lam):
        assert np.array_equal(t, t.T)
        assert abs(q @ np.diag(lam) @ q.T - t).max() <= 1e-13 * max(abs(t).max(), top)


def test_exactly_one_zeroed_mode(case):
    _, _, _, factors = case
    sums = factors.sums()
    assert factors.null_threshold == 1e-12 * abs(sums).max()
    assert factors.zeroed == 1 and int((abs(sums) <= factors.null_threshold).sum()) == 1
    mult = factors.multipliers()
    assert int((mult == 0.0).sum()) == 1 and np.isfinite(mult).all()


# ---- 2. the numpy restatement -------------------------------------------------------------------------------------------
def test_restatement_solves_the_projection(case):
    s, Lp, C, factors = case
    vel = np.random.default_rng(3).standard_normal(s.n_u)
    rhs = s.B @ vel
    phi = factors.solve(rhs)
    res = np.linalg.norm(Lp @ phi - rhs) / np.linalg.norm(rhs)
    div = np.linalg.norm(s.B @ (vel - C @ phi)) / np.linalg.norm(rhs)
    mean = abs(phi.mean()) / abs(phi).max()
    print("residual %.3g  |B (vel - C phi)| / |B vel| %.3g  |mean phi| / max |phi| %.3g" % (res, div, mean))
    assert res <= 1e-13
    assert div <= 1e-13
    assert mean <= 1e-13
    phi_cg, its = jacobi_cg(Lp, rhs, 1e-13)
    diff = np.linalg.norm(C @ phi - C @ phi_cg) / np.linalg.norm(vel)
    shift = phi - phi_cg                                   # phi itself differs by a constant
    print("Jacobi-CG: %d iterations, |C phi - C phi_cg| / |vel| %.3g, phi - phi_cg = %.3g +- %.3g"
          % (its, diff, shift.mean(), np.ptp(shift)))
    assert diff <= 1e-10


# ---- 3. the declines ----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lp_3d_n4():
    s = system_of("3d_n4")
    return s, projection_operators(s)[0]


def test_declines_a_perturbed_operator(lp_3d_n4):
    from hipla.fdm import fdm_factors
    s, Lp = lp_3d_n4
    bad = Lp.tolil(copy=True)
    r, c = 21, 22                                          # a stored off-diagonal pair away from the origin's lines
    assert bad[r, c] != 0.0
    bad[r, c] += 1e-6
    bad[c, r] += 1e-6
    factors, why = fdm_factors(bad.tocsr(), (s.n,) * s.dim)
    assert factors is None and isinstance(why, str) and why
    bad = Lp.tolil(copy=True)                              # ... and one ON the line through the origin along x
    bad[0, 1] += 1e-6
    bad[1, 0] += 1e-6
    factors, why = fdm_factors(bad.tocsr(), (s.n,) * s.dim)
    assert factors is None and isinstance(why, str) and why


def test_declines_a_permuted_operator(lp_3d_n4):
    from hipla.fdm import fdm_factors
    s, Lp = lp_3d_n4
    perm = np.random.default_rng(5).permutation(s.n_p)
    factors, why = fdm_factors(Lp[perm][:, perm].tocsr(), (s.n,) * s.dim)
    assert factors is None and isinstance(why, str) and why


@pytest.mark.parametrize("extents", [(4, 4), (4, 4, 5), (2, 8, 4), (64,), (4, 4, 2, 2), (0, 4, 16), (8, 8)])
def test_declines_wrong_extents(lp_3d_n4, extents):
    from hipla.fdm import fdm_factors
    _, Lp = lp_3d_n4
    factors, why = fdm_factors(Lp, extents)
    assert factors is None and isinstance(why, str) and why


def test_try_create_keeps_the_reason(numpy_engine, lp_3d_n4):
    import hipla
    s, Lp = lp_3d_n4
    assert hipla.FastDiagonalization.try_create(Lp, (4, 4, 5)) is None
    assert isinstance(hipla.FastDiagonalization.last_declined, str)
    with pytest.raises(ValueError):
        hipla.FastDiagonalization(Lp, (4, 4, 5))
    inv = hipla.FastDiagonalization.try_create(Lp, (s.n,) * s.dim)
    assert inv is not None and hipla.FastDiagonalization.last_declined is None
    assert inv.iterations == 0 and inv.handle is None and inv.height == inv.width == s.n_p
    inv.precision, inv.maxsteps = 1e-3, 1                  # there to be set, and ignored
    rhs = s.B @ np.random.default_rng(1).standard_normal(s.n_u)
    y = hipla.Vector(s.n_p)
    y.data = inv * hipla.Vector.from_numpy(rhs)
    assert np.array_equal(y.numpy(), inv.factors.solve(rhs)) and inv.iterations == 0


# ---- 4. the template ----------------------------------------------------------------------------------------------------
GRIDS = {"2d": (2, 5), "3d": (3, 4)}
TAU = 0.05


def fresh(grid, time_scheme="euler"):
    """A `NavierStokes` with a seeded divergence-free start, a seeded force and the velocity solve run to 1e-13."""
    import hipla
    from templates.NavierStokesSIMPLE_iterative import NavierStokes, SyntheticMesh
    dim, n = GRIDS[grid]
    ns = NavierStokes(SyntheticMesh(1.0 / n, dim=dim), nu=0.01, inflow="inlet", outflow="outlet", wall="wall|cyl",
                      uin=None, timestep=TAU, order=0, time_scheme=time_scheme)
    s = ns.system
    ns.f.vec.data = hipla.Vector.from_numpy(0.1 * np.random.default_rng(8).standard_normal(s.n_u))
    u0 = 0.2 * kr.project(s.B, np.full(s.n_u, s.h ** s.dim), np.random.default_rng(2).standard_normal(s.n_u))[0]
    ns.gfu.data = hipla.Vector.from_numpy(u0)
    held, name = ns._momentum_solver()
    held[name].precision, held[name].maxsteps = 1e-13, 5000
    return ns


def twins(grid, time_scheme="euler"):
    """(the "fdm" object, the "cg" object with its projection run to 1e-13)."""
    direct, cg = fresh(grid, time_scheme), fresh(grid, time_scheme)
    direct.SetProjection("fdm")
    ops = cg._time_stepping_operators()
    ops["invproj"].precision, ops["invproj"].maxsteps = 1e-13, 20000
    return direct, cg


def quiet(call, *args, **kw):
    with contextlib.redirect_stdout(io.StringIO()):
        return call(*args, **kw)


def rel(a, b):
    return np.linalg.norm(np.asarray(a) - b) / np.linalg.norm(b)


def spy_on_project(ns):
    """|B vel| of every velocity `ns.Project` is handed, in order."""
    seen, inner = [], ns.Project

    def project(vel):
        seen.append(np.linalg.norm(ns.system.B @ vel.numpy()))
        inner(vel)
    ns.Project = project
    return seen


@pytest.mark.parametrize("grid", sorted(GRIDS))
@pytest.mark.parametrize("time_scheme", ["euler", "cnab2"])
def test_do_time_step_follows_the_switch(numpy_engine, grid, time_scheme):
    import hipla
    direct, cg = twins(grid, time_scheme)
    assert direct.projection == "fdm" and cg.projection == "cg"
    assert isinstance(direct._time_stepping_operators()["invproj"], hipla.FastDiagonalization)
    raws = spy_on_project(direct)
    B = direct.system.B
    for step in range(3):
        quiet(direct.DoTimeStep)
        quiet(cg.DoTimeStep)
        raw = np.linalg.norm(B @ direct.last_stages["raw"].numpy()) if time_scheme == "cnab2" else raws[-1]
        div = np.linalg.norm(B @ direct.gfu.numpy())
        err = rel(direct.gfu.numpy(), cg.gfu.numpy())
        print("step %d: |u_fdm - u_cg| / |u| %.3g  |B u| %.3g  |B raw| %.3g" % (step, err, div, raw))
        assert err <= 1e-9
        assert div <= 1e-12 * raw
        assert direct._time_stepping_operators()["invproj"].iterations == 0
    shift = direct.gfup.numpy() - cg.gfup.numpy()          # the potential differs by a constant, and by no more
    assert np.ptp(shift) <= 1e-8 * abs(cg.gfup.numpy()).max()


@pytest.mark.parametrize("grid", sorted(GRIDS))
def test_project_follows_the_switch(numpy_engine, grid):
    import hipla
    direct, cg = twins(grid)
    vel = np.random.default_rng(11).standard_normal(direct.system.n_u)
    out = []
    for ns in (direct, cg):
        v = hipla.Vector.from_numpy(vel)
        quiet(ns.Project, v)
        out.append(v.numpy())
    B = direct.system.B
    err, div, raw = rel(out[0], out[1]), np.linalg.norm(B @ out[0]), np.linalg.norm(B @ vel)
    print("|v_fdm - v_cg| / |v| %.3g  |B v| %.3g  |B raw| %.3g" % (err, div, raw))
    assert err <= 1e-9
    assert div <= 1e-12 * raw
    assert abs(direct.gfup.numpy().mean()) <= 1e-13 * abs(direct.gfup.numpy()).max()


@pytest.mark.parametrize("grid", sorted(GRIDS))
@pytest.mark.parametrize("time_scheme", ["euler", "cnab2"])
def test_advance_by_statements_follows_the_switch(numpy_engine, grid, time_scheme):
    direct, cg = twins(grid, time_scheme)
    sizes = [0.05, 0.03, 0.04]
    rec = quiet(direct.Advance, 3, timesteps=sizes, precision=(1e-13, 1e-3), maxsteps=(5000, 1))
    ref = quiet(cg.Advance, 3, timesteps=sizes, precision=(1e-13, 1e-13), maxsteps=(5000, 20000))
    assert rec.declined is not None and rec.projection == "fdm" and ref.projection == "cg"
    assert (rec.proj_iterations == 0).all() and (ref.proj_iterations > 0).all()
    err = rel(direct.gfu.numpy(), cg.gfu.numpy())
    print("|u_fdm - u_cg| / |u| %.3g  div_norm %s" % (err, rec.div_norm))
    assert err <= 1e-9
    assert np.array_equal(rec.timestep, sizes)


def test_set_projection_cg_restores_the_solver(numpy_engine):
    import hipla
    ns = fresh("2d")
    original = ns._time_stepping_operators()["invproj"]
    assert isinstance(original, hipla.CGSolver)
    ns.SetProjection("fdm")
    made = ns._time_stepping_operators()["invproj"]
    assert isinstance(made, hipla.FastDiagonalization) and ns.projection == "fdm"
    ns.SetProjection("fdm")
    assert ns._time_stepping_operators()["invproj"] is made          # built once
    ns.SetProjection("cg")
    assert ns._time_stepping_operators()["invproj"] is original and ns.projection == "cg"
    ns.SetProjection("fdm")
    assert ns._time_stepping_operators()["invproj"] is made


def test_the_default_builds_no_fast_diagonalization(numpy_engine, monkeypatch):
    import hipla
    from hipla import fdm
    built = []
    monkeypatch.setattr(fdm, "fdm_factors", lambda *a, **k: built.append(a) or (None, "not in this test"))
    ns = fresh("2d")
    assert ns.projection == "cg"
    quiet(ns.DoTimeStep)
    rec = quiet(ns.Advance, 1)
    ns.SetProjection("cg")
    assert rec.projection == "cg" and not built and ns._fdm is None
    assert type(ns._time_stepping_operators()["invproj"]) is hipla.CGSolver


def test_set_projection_refuses_other_names(numpy_engine):
    ns = fresh("2d")
    with pytest.raises(ValueError):
        ns.SetProjection("x")
    assert ns.projection == "cg" and ns._fdm is None


def test_set_projection_raises_the_reason(numpy_engine, monkeypatch):
    from hipla import fdm
    ns = fresh("2d")
    monkeypatch.setattr(fdm, "fdm_factors", lambda *a, **k: (None, "not a Kronecker sum in this test"))
    with pytest.raises(ValueError, match="not a Kronecker sum in this test"):
        ns.SetProjection("fdm")
    assert ns.projection == "cg"
