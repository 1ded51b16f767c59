"""The direct velocity and scalar solves by fast diagonalisation on the host (no GPU): `hipla.component_factors` on the
grids of this package, the numpy restatement `ComponentFactors.solve` against scipy's sparse LU, the declines, and
`NavierStokes.SetImplicitSolve` on the CPU checker engine.

Bounds.  The restatement: residual <= max(10 x the residual of the LU solution, 1e-14) |rhs| (the restatement is a
dense orthogonal transform, a division and the transform back: backward stable like the LU; measured 9e-16 to 2e-15
against 1e-16 to 4e-16).  The template: 1e-9 |u| against a twin whose velocity and scalar CG run to 1e-12 and 1e-14, both
with the projection's CG at 1e-13 -- the twin's own CG error."""

import contextlib
import io

import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spla

from oracle import krylov_ref as kr

GRIDS = [(2, 2), (2, 3), (2, 8), (3, 2), (3, 5), (3, 9)]
SIGMAS = [0.0, 1e-3, 0.37, 50.0]
WALLS = {"x-": 1.0, "x+": 0.0}


def velocity_case(dim, n):
    from staggered_grid import mac_stokes
    s = mac_stokes(dim, n, 0.01)
    return s.A, s.component_ids, np.full(s.n_u, s.h ** s.dim)


def scalar_case(dim, n):
    from staggered_grid import mac_stokes
    s = mac_stokes(dim, n, 0.01)
    ops = s.scalar_operators(0.8, WALLS)
    return sp.csr_matrix(ops["K"]), [np.arange(s.n_p).reshape((n,) * dim)], np.asarray(ops["mass"], dtype=np.float64)


CASES = {"u%dd_n%d" % g: (velocity_case, g) for g in GRIDS}
CASES.update({"T2d_n8": (scalar_case, (2, 8)), "T3d_n5": (scalar_case, (3, 5))})


@pytest.fixture(scope="module", params=sorted(CASES))
def case(request):
    from hipla.fdm import component_factors
    make, grid = CASES[request.param]
    mat, comps, mass = make(*grid)
    factors, why = component_factors(mat, comps, mass)
    assert why is None and factors is not None, why
    return grid, mat, comps, mass, factors


# ---- 1. the factors ---------------------------------------------------------------------------------------------------
def test_factors_describe_the_layout(case):
    (dim, n), mat, comps, mass, cf = case
    assert cf.n_total == mat.shape[0] and cf.dim == dim and len(cf.factors) == len(comps)
    assert [f.extents for f in cf.factors] == [g.shape for g in comps] and cf.extents == [g.shape for g in comps]
    nnz = 0
    for g, base, f, m in zip(comps, cf.bases, cf.factors, cf.masses):
        k = np.arange(g.shape[0]).reshape((-1,) + (1,) * (dim - 1))
        inside = np.arange(int(np.prod(g.shape[1:]))).reshape(g.shape[1:])
        assert np.array_equal(g, base + k * cf.pitch + inside)          # the layout the kernel addresses
        assert f.error <= 1e-12 and m == mass[g.flat[0]] and m > 0.0     # (the bound `fdm_factors` declines at)
        nnz += mat[g.ravel()][:, g.ravel()].nnz
        sums = f.sums()
        assert sums.min() > 0.0                                          # single eigenvalues may be negative; no sum is
    assert nnz == mat.nnz                                                # no entry couples two components
    if len(comps) > 1:
        assert cf.pitch == (2 * n - 1 if dim == 2 else 3 * n * n - 2 * n)


# ---- 2. the restatement against LU ------------------------------------------------------------------------------------
@pytest.mark.parametrize("sigma", SIGMAS)
def test_restatement_against_sparse_lu(case, sigma):
    _, mat, _, mass, cf = case
    rhs = np.random.default_rng(5).standard_normal(cf.n_total)
    op = (sp.diags(mass) + sigma * mat).tocsc()
    x_lu = spla.splu(op).solve(rhs)
    size = np.linalg.norm(rhs)
    res_lu = np.linalg.norm(op @ x_lu - rhs) / size
    x = cf.solve(rhs, sigma)
    res = np.linalg.norm(op @ x - rhs) / size
    print("sigma %g: residual %.3g (LU %.3g)" % (sigma, res, res_lu))
    assert res <= max(10 * res_lu, 1e-14)
    assert x is not rhs and not np.shares_memory(x, rhs)


# ---- 3. the declines --------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sys_3d_n5():
    from staggered_grid import mac_stokes
    s = mac_stokes(3, 5, 0.01)
    return s, np.full(s.n_u, s.h ** s.dim)


def declined(mat, comps, mass, word):
    from hipla.fdm import component_factors
    factors, why = component_factors(mat, comps, mass)
    assert factors is None and isinstance(why, str) and word in why, why
    return why


def test_declines_an_inflated_system(sys_3d_n5):
    s, m = sys_3d_n5
    big = s.inflate(3)
    declined(big.A, big.component_ids, np.full(big.A.shape[0], m[0]), "miss")


def test_declines_a_permuted_system(sys_3d_n5):
    s, m = sys_3d_n5
    moved = s.permuted(np.random.default_rng(5).permutation(s.n_u))
    declined(moved.A, moved.component_ids, m, "one to three")           # it carries no component ids
    declined(moved.A, s.component_ids, m, "couples")                    # ... and with the grid's, its entries do not fit


def test_declines_a_coupling_entry(sys_3d_n5):
    s, m = sys_3d_n5
    bad = s.A.tolil(copy=True)
    r, c = int(s.component_ids[0][1, 1, 1]), int(s.component_ids[2][1, 1, 1])
    assert bad[r, c] == 0.0
    bad[r, c] = 1e-3
    why = declined(bad.tocsr(), s.component_ids, m, "couples")
    assert "(%d, %d)" % (r, c) in why


def test_declines_a_non_uniform_mass(sys_3d_n5):
    s, m = sys_3d_n5
    bad = m.copy()
    bad[int(s.component_ids[1][2, 1, 3])] *= 1.5
    declined(s.A, s.component_ids, bad, "mass")
    declined(s.A, s.component_ids, -m, "mass")
    from hipla.fdm import component_factors
    per_component = m.copy()                                            # constant on each component is enough
    per_component[s.component_ids[2].ravel()] *= 2.0
    factors, why = component_factors(s.A, s.component_ids, per_component)
    assert why is None and factors.masses == [m[0], m[0], 2.0 * m[0]]


def test_declines_components_that_miss_a_row(sys_3d_n5):
    s, m = sys_3d_n5
    declined(s.A, s.component_ids[:2], m, "miss")
    short = [s.component_ids[0], s.component_ids[1], s.component_ids[2][:, :, :-1]]
    declined(s.A, short, m, "")                                         # (not affine any more, or rows missed)


def test_declines_ids_that_are_not_affine(sys_3d_n5):
    s, m = sys_3d_n5
    swapped = [g.copy() for g in s.component_ids]
    swapped[0][0, 0, 0], swapped[0][0, 0, 1] = swapped[0][0, 0, 1], swapped[0][0, 0, 0]
    declined(s.A, swapped, m, "affine")
    declined(s.A, [g.astype(np.float64) for g in s.component_ids], m, "integer")
    declined(s.A.toarray(), s.component_ids, m, "sparse")


def test_declines_a_perturbed_component(sys_3d_n5):
    """An entry inside one component that no Kronecker sum has: the reason of `fdm_factors` is passed on."""
    s, m = sys_3d_n5
    g = s.component_ids[1]
    bad = s.A.tolil(copy=True)
    r, c = int(g[2, 1, 1]), int(g[2, 1, 2])
    assert bad[r, c] != 0.0
    bad[r, c] += 1e-6
    bad[c, r] += 1e-6
    declined(bad.tocsr(), s.component_ids, m, "component 1: ")


def test_try_create_keeps_the_reason(numpy_engine, sys_3d_n5):
    import hipla
    s, m = sys_3d_n5
    cls = hipla.ComponentFastDiagonalization
    assert cls.try_create(s.A, s.component_ids[:2], m, 0.1) is None and "miss" in cls.last_declined
    with pytest.raises(ValueError, match="miss"):
        cls(s.A, s.component_ids[:2], m, 0.1)
    inv = cls.try_create(s.A, s.component_ids, m, 0.1)
    assert inv is not None and cls.last_declined is None and hipla.FastDiagonalization.last_declined != "x"
    assert inv.iterations == 0 and inv.handle is None and inv.height == inv.width == s.n_u and inv.sigma == 0.1
    inv.precision, inv.maxsteps = 1e-3, 1                               # there to be set, and ignored
    rhs = np.random.default_rng(1).standard_normal(s.n_u)
    y = hipla.Vector(s.n_u)
    y.data = inv * hipla.Vector.from_numpy(rhs)
    assert np.array_equal(y.numpy(), inv.factors.solve(rhs, 0.1)) and inv.iterations == 0
    inv.sigma = 0.025
    y.data = inv * hipla.Vector.from_numpy(rhs)
    assert np.array_equal(y.numpy(), inv.factors.solve(rhs, 0.025))
    for bad in (-1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            inv.sigma = bad
    assert inv.sigma == 0.025


# ---- 4. the template --------------------------------------------------------------------------------------------------
TAU = 0.05
TEMPLATE_GRIDS = {"2d": (2, 5, (0.0, 2.0)), "3d": (3, 4, (0.0, 2.0, -1.0))}


def fresh(grid, time_scheme="euler", buoyant=False, order=0):
    """A `NavierStokes` with a seeded divergence-free start and force, the projection's CG at 1e-13, the velocity's (and
    the scalar's) CG at 1e-12 (1e-14)."""
    import hipla
    from templates.NavierStokesSIMPLE_iterative import NavierStokes, SyntheticMesh
    dim, n, beta = TEMPLATE_GRIDS[grid]
    ns = NavierStokes(SyntheticMesh(1.0 / n, dim=dim), nu=0.01, inflow="inlet", outflow="outlet", wall="wall|cyl",
                      uin=None, timestep=TAU, order=order, time_scheme=time_scheme)
    s = ns.system
    if order == 0:
        ns.f.vec.data = hipla.Vector.from_numpy(0.1 * np.random.default_rng(8).standard_normal(s.n_u))
        u0 = 0.2 * kr.project(s.B, np.full(s.n_u, s.h ** s.dim), np.random.default_rng(2).standard_normal(s.n_u))[0]
        ns.gfu.data = hipla.Vector.from_numpy(u0)
    if buoyant:
        ns.AddScalar(initial=np.random.default_rng(6).random(s.n_p), precision=1e-14, maxsteps=5000, kappa=0.8,
                     dirichlet=WALLS, buoyancy=beta, t_ref=0.5)
    held, name = ns._momentum_solver()
    held[name].precision, held[name].maxsteps = 1e-12, 5000
    ops = ns._time_stepping_operators()
    ops["invmstar"].precision, ops["invmstar"].maxsteps = 1e-12, 5000
    ops["invproj"].precision, ops["invproj"].maxsteps = 1e-13, 20000
    return ns


def quiet(call, *args, **kw):
    with contextlib.redirect_stdout(io.StringIO()):
        return call(*args, **kw)


def rel(a, b):
    return np.linalg.norm(np.asarray(a) - b) / np.linalg.norm(b)


def test_set_implicit_solve_refuses_other_names(numpy_engine):
    ns = fresh("2d")
    with pytest.raises(ValueError, match="cg"):
        ns.SetImplicitSolve("lu")
    assert ns.implicit_solve == "cg" and ns._fdm_u is None


def test_set_implicit_solve_raises_the_reason_for_an_inflated_system(numpy_engine):
    ns = fresh("2d", order=1)
    assert ns.system.block_size > 1
    with pytest.raises(ValueError, match="SetImplicitSolve"):
        ns.SetImplicitSolve("fdm")
    assert ns.implicit_solve == "cg" and ns._fdm_u is None


@pytest.mark.parametrize("grid", sorted(TEMPLATE_GRIDS))
@pytest.mark.parametrize("time_scheme", ["euler", "cnab2"])
@pytest.mark.parametrize("buoyant", [False, True])
def test_do_time_step_follows_the_switch(numpy_engine, grid, time_scheme, buoyant):
    import hipla
    direct, cg = fresh(grid, time_scheme, buoyant), fresh(grid, time_scheme, buoyant)
    direct.SetImplicitSolve("fdm")
    assert direct.implicit_solve == "fdm" and cg.implicit_solve == "cg"
    assert isinstance(direct._fdm_u, hipla.ComponentFastDiagonalization) and not direct._by_step
    for size in (None, 0.03, None):
        quiet(direct.DoTimeStep, size)
        quiet(cg.DoTimeStep, size)
        assert direct._last_momentum_solver is direct._fdm_u and direct._fdm_u.iterations == 0
        assert direct._fdm_u.sigma == (0.5 if time_scheme == "cnab2" else 1.0) * (TAU if size is None else size)
        err = rel(direct.gfu.numpy(), cg.gfu.numpy())
        print("step of %s: |u_fdm - u_cg| / |u| %.3g" % (size, err))
        assert err <= 1e-9
        if buoyant:
            assert rel(direct.temperature.numpy(), cg.temperature.numpy()) <= 1e-9
            assert direct._scalar.last_solver is direct._scalar.shared["fdm_T"]
    assert not direct._by_step                                          # nothing is kept by step size


def test_scalar_added_after_the_switch_follows_it(numpy_engine):
    import hipla
    ns = fresh("2d")
    ns.SetImplicitSolve("fdm")
    ns.AddScalar(kappa=0.8, dirichlet=WALLS, buoyancy=(0.0, 2.0), t_ref=0.5)
    assert ns._scalar.implicit == "fdm"
    assert isinstance(ns._scalar.shared["fdm_T"], hipla.ComponentFastDiagonalization)
    ns.SetImplicitSolve("cg")
    assert ns._scalar.implicit == "cg" and ns._scalar.solver_for(None) is ns._scalar.inv


@pytest.mark.parametrize("time_scheme", ["euler", "cnab2"])
def test_advance_by_statements_and_pseudo_follow_the_switch(numpy_engine, time_scheme):
    direct, cg = fresh("2d", time_scheme, True), fresh("2d", time_scheme, True)
    direct.SetImplicitSolve("fdm")
    sizes = [0.05, 0.03, 0.04]
    rec = quiet(direct.Advance, 3, timesteps=sizes, precision=(1e-3, 1e-13), maxsteps=(1, 20000))
    ref = quiet(cg.Advance, 3, timesteps=sizes, precision=(1e-12, 1e-13), maxsteps=(5000, 20000))
    assert rec.declined is not None and rec.implicit == "fdm" and ref.implicit == "cg"
    assert (rec.mstar_iterations == 0).all() and (rec.scalar_iterations == 0).all() and (ref.mstar_iterations > 0).all()
    assert rel(direct.gfu.numpy(), cg.gfu.numpy()) <= 1e-9
    assert rel(direct.temperature.numpy(), cg.temperature.numpy()) <= 1e-9
    # the pseudo time stepping projects a velocity that is divergence-free already: B u is rounding noise with a
    # component along the constants, on which a CG projection does not converge (tests/test_fdm_gpu.py) -- both
    # objects take the direct projection, so that the velocity solves are what differs
    direct, cg = fresh("2d", time_scheme), fresh("2d", time_scheme)
    direct.SetImplicitSolve("fdm")
    direct.SetProjection("fdm")
    cg.SetProjection("fdm")
    rec = quiet(direct.Advance, 2, pseudo=True, precision=(1e-3, 1e-13), maxsteps=(1, 20000))
    quiet(cg.Advance, 2, pseudo=True, precision=(1e-12, 1e-13), maxsteps=(5000, 20000))
    assert (rec.mstar_iterations == 0).all() and direct._fdm_u.sigma == TAU
    assert rel(direct.gfu.numpy(), cg.gfu.numpy()) <= 1e-9


@pytest.mark.parametrize("time_scheme", ["euler", "cnab2"])
def test_back_at_cg_the_bits_are_the_default_ones(numpy_engine, time_scheme):
    def run(switch):
        import hipla
        from templates.NavierStokesSIMPLE_iterative import NavierStokes, SyntheticMesh
        ns = NavierStokes(SyntheticMesh(0.2, dim=2), nu=0.01, inflow="inlet", outflow="outlet", wall="wall|cyl",
                          uin=None, timestep=TAU, order=0, time_scheme=time_scheme)
        s = ns.system
        ns.f.vec.data = hipla.Vector.from_numpy(0.1 * np.random.default_rng(8).standard_normal(s.n_u))
        ns.AddScalar(initial=np.random.default_rng(6).random(s.n_p), kappa=0.8, dirichlet=WALLS, buoyancy=(0.0, 2.0))
        if switch:
            ns.SetImplicitSolve("fdm")
            ns.SetImplicitSolve("cg")
        quiet(ns.DoTimeStep)
        quiet(ns.DoTimeStep, 0.03)
        rec = quiet(ns.Advance, 2)
        return ns.gfu.numpy(), ns.gfup.numpy(), ns.temperature.numpy(), rec.mstar_iterations
    for a, b in zip(run(False), run(True)):
        assert np.array_equal(a, b)
