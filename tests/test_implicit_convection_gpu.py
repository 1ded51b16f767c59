"""Linearly implicit convection on the product engine: the flux and the rows of form (ii) of the BiCGStab loop and its
point-Jacobi diagonal against numpy on operands no grid produces, form (ii) on grids against `spsolve`, and
`Advance` / `DoTimeStep` after `SetConvectionTreatment("implicit")` against the numpy reference step
(tests/implicit_convection_reference.py).

Bounds.  Kernels against numpy: 1e-13 of the scale of the terms, the bound tests/test_step_kernels_gpu.py holds
`nss_step_rhs_f64` and the flux kernel to (its helpers are used here).  Solves at 1e-12 against `spsolve` and steps
against the reference: 1e-9 relative, the project's bound for such twins (tests/test_implicit_fdm_gpu.py).  `Advance`
against `DoTimeStep` repeated: 1e-8, the bound of tests/test_time_stepper_gpu.py for those two paths.  `==` where the
same launches run."""

import contextlib
import io

import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spl

import implicit_convection_reference as icr
from oracle import krylov_ref as kr
from test_step_kernels_gpu import SENT, TOL, absvec, matvec, two_slot

pytestmark = pytest.mark.gpu

TAU = 0.05
WALLS = {"x-": 1.0, "x+": 0.0}
GRIDS = {"2d": (2, 8, (0.0, 2.0)), "3d": (3, 5, (0.0, 2.0, -1.0))}
SIZES = [0.05, 0.2, 0.1, 0.02]
TIGHT = dict(precision=(1e-12, 1e-13), maxsteps=(4000, 20000))
MODES = {"fixed": lambda k: {}, "timesteps": lambda k: dict(timesteps=SIZES[k]),
         "cfl": lambda k: dict(cfl=4.0, max_timestep=10.0)}


def rel(a, b):
    return np.linalg.norm(np.asarray(a) - b) / np.linalg.norm(b)


def quiet(call, *args, **kw):
    with contextlib.redirect_stdout(io.StringIO()):
        return call(*args, **kw)


# ---- 1. the flux and the rows of form (ii), the Jacobi diagonal ---------------------------------------------------------
def random_rows(rng, n, width, most):
    """Random (n, width) CSR with 0 .. `most` entries per row."""
    counts = rng.integers(0, most + 1, size=n)
    indptr = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    cols = rng.integers(0, max(1, width), size=int(indptr[-1])).astype(np.int32)
    mat = sp.csr_matrix((rng.standard_normal(cols.size), cols, indptr), shape=(n, max(1, width)))
    mat.sum_duplicates()
    mat.sort_indices()
    return mat[:, :width] if width else sp.csr_matrix((n, 0))


def form_two(eng, rng, nflux, uniform):
    """A form-(ii) loop on random operands: (loop, host operands)."""
    import hipla
    from hipla.fused import BicgstabLoop, ConvectiveForm
    n = 2 * nflux // 3 + 5
    L, Dv = random_rows(rng, n, n, 4), random_rows(rng, n, nflux, 3)
    rows = sp.hstack([L, Dv], format="csr")
    rows.sort_indices()
    counts = ([2], [1]) if nflux == 1 else (None, None)       # (one flux point: a live row in each)
    avg, dif = two_slot(rng, nflux, n, counts[0]), two_slot(rng, nflux, n, counts[1])
    a = rng.standard_normal(nflux)
    a[::7] = 0.0
    a[3::7] = -0.0
    mass = np.full(n, 5.5) if uniform else 5.0 + rng.random(n)
    form = ConvectiveForm(hipla.SparseMatrix.from_scipy(rows), hipla.SparseMatrix.from_scipy(avg),
                          hipla.SparseMatrix.from_scipy(dif), eng.from_host(a), ConvectiveForm.mass_operand(eng, mass))
    assert (form.mass[0] is None) == uniform
    loop = BicgstabLoop(eng, form.rows, form=form)
    return loop, dict(n=n, L=L, Dv=Dv, rows=rows, avg=avg, dif=dif, a=a, mass=mass)


@pytest.mark.parametrize("uniform", [True, False])
@pytest.mark.parametrize("nflux", [1, 63, 64, 65, 257, 1025])
def test_flux_and_rows_of_form_two(hip_engine, nflux, uniform):
    eng = hip_engine
    rng = np.random.default_rng(10 * nflux + uniform)
    loop, h = form_two(eng, rng, nflux, uniform)
    n, sigma = h["n"], 0.3
    loop.set_sigma(sigma)
    v = rng.standard_normal(n)
    if nflux > 1:
        assert (h["a"] > 0).any() and (h["a"] < 0).any() and np.signbit(h["a"][3]) and h["a"][0] == 0.0
    operand = eng.from_host(np.concatenate([v, np.full(nflux, SENT)]))
    y = eng.from_host(np.full(n + 1, SENT))
    loop.apply(operand, y)
    got_op, got_y = eng.to_host(operand), eng.to_host(y)
    assert np.array_equal(got_op[:n], v) and got_y[-1] == SENT
    m, d = matvec(h["avg"], v), matvec(h["dif"], v)
    want_F = np.asarray(h["a"] * m - np.abs(h["a"]) * d / 2, dtype=np.float64)
    scale_F = np.abs(h["a"]) * (absvec(h["avg"], v) + absvec(h["dif"], v) / 2)
    err_F = np.abs(got_op[n:] - want_F)
    assert (err_F <= TOL * scale_F).all(), err_F.max()
    assert (got_op[n:][h["a"] == 0.0] == 0.0).all()                             # +0.0 and -0.0 advect nothing
    full = np.concatenate([v, got_op[n:]])                                       # the rows, from the flux the device formed
    want_y = np.asarray(h["mass"] * v + sigma * matvec(h["rows"], full), dtype=np.float64)
    scale_y = np.abs(h["mass"] * v) + sigma * absvec(h["rows"], full)
    err_y = np.abs(got_y[:n] - want_y)
    print("nflux = %d: flux %.3g, rows %.3g of the scale" % (nflux, (err_F[scale_F > 0] / scale_F[scale_F > 0]).max(initial=0),
                                                              (err_y / scale_y).max()))
    assert (err_y <= TOL * scale_y).all(), err_y.max()
    # with the done word set nothing is written
    loop.ctrl[0] = 1
    operand2, y2 = eng.from_host(np.concatenate([v, np.full(nflux, SENT)])), eng.from_host(np.full(n + 1, SENT))
    loop.apply(operand2, y2)
    assert (eng.to_host(operand2)[n:] == SENT).all() and (eng.to_host(y2) == SENT).all()
    loop.ctrl[0] = 0


@pytest.mark.parametrize("uniform", [True, False])
@pytest.mark.parametrize("nflux", [1, 64, 65, 1025])
def test_jacobi_diagonal_of_form_two(hip_engine, nflux, uniform):
    eng = hip_engine
    rng = np.random.default_rng(77 * nflux + uniform)
    loop, h = form_two(eng, rng, nflux, uniform)
    n, sigma, a = h["n"], 0.3, h["a"]
    loop.set_sigma(sigma)
    dinv = eng.from_host(np.full(n + 1, SENT))
    loop.write_jacobi(dinv)
    got = eng.to_host(dinv)
    assert got[-1] == SENT
    N = h["Dv"] @ (sp.diags(a) @ h["avg"] - 0.5 * sp.diags(np.abs(a)) @ h["dif"])
    want = h["mass"] + sigma * (h["L"].diagonal() + N.diagonal())
    scale = h["mass"] + sigma * (np.abs(h["L"].diagonal())
                                 + (abs(h["Dv"]) @ (sp.diags(np.abs(a)) @ (abs(h["avg"]) + 0.5 * abs(h["dif"])))).diagonal())
    err = np.abs(1.0 / got[:n] - want)
    print("nflux = %d: diagonal %.3g of the scale" % (nflux, (err / scale).max()))
    assert (err <= TOL * scale).all(), err.max()


# ---- 2. form (ii) on grids against spsolve ----------------------------------------------------------------------------------
@pytest.mark.parametrize("pre", ["none", "jacobi", "fdm"])
@pytest.mark.parametrize("dim,n", [(2, 4), (2, 5), (3, 3), (3, 4)])
def test_form_two_on_grids_against_spsolve(hip_engine, dim, n, pre):
    import hipla
    from hipla.stepping import LinearisedConvection
    from staggered_grid import mac_stokes
    s = mac_stokes(dim, n, 0.01)
    m_u = np.full(s.n_u, s.h ** s.dim)
    u = kr.project(s.B, m_u, np.random.default_rng(2).standard_normal(s.n_u))[0]
    rate = ((abs(s.B) @ np.abs(u)) / s.mass).max()
    u *= 4.0 / (TAU * rate)                                                      # tau * CflRate = 4
    op = LinearisedConvection(s.convection_operators(), m_u, s.A, sigma=TAU)
    op.freeze(hipla.Vector.from_numpy(u))
    P = None
    if pre == "jacobi":
        P = op.jacobi()
        assert np.allclose(hip_engine.to_host(P.d), 1.0 / op.to_scipy().diagonal(), rtol=1e-13, atol=0.0)
    elif pre == "fdm":
        P = hipla.ComponentFastDiagonalization.try_create(s.A, s.component_ids, m_u, TAU)
        assert P is not None and P.handle is not None
    inv = hipla.BiCGStabSolver(op, P, precision=1e-12, maxsteps=2000)
    b = np.random.default_rng(1).standard_normal(s.n_u)
    x = hipla.Vector(s.n_u)
    x.data = inv * hipla.Vector.from_numpy(b)
    assert inv._fused is not None and inv._fused.form is not None, hipla.fused.BicgstabLoop.last_declined
    M = icr.momentum_operator(s, s.convection_operators()["adv"] @ u, TAU)
    y = hipla.Vector(s.n_u)
    y.data = op * hipla.Vector.from_numpy(b)
    assert rel(y.numpy(), M @ b) <= 1e-13                                        # the operator is the assembled one
    ref = spl.spsolve(M, b)
    print("%d-D n = %d, %s: %d iterations, %.3g from spsolve" % (dim, n, pre, inv.iterations, rel(x.numpy(), ref)))
    assert 0 < inv.iterations < 2000 and rel(x.numpy(), ref) <= 1e-9


# ---- 3. the steps against the reference ---------------------------------------------------------------------------------------
def fresh(grid, buoyant=False, projection=None, implicit=None, treatment="implicit"):
    """The set-up of tests/test_implicit_fdm_gpu.py (the scalar's solve at 1e-12: a BiCGStab residual)."""
    import hipla
    from templates.NavierStokesSIMPLE_iterative import NavierStokes, SyntheticMesh
    dim, n, beta = GRIDS[grid]
    ns = NavierStokes(SyntheticMesh(1.0 / n, dim=dim), nu=0.01, inflow="inlet", outflow="outlet", wall="wall|cyl",
                      uin=None, timestep=TAU, order=0)
    s = ns.system
    assert s.block_size == 1 and s.n == n
    ns.f.vec.data = hipla.Vector.from_numpy(0.5 * s.h ** s.dim * np.random.default_rng(8).standard_normal(s.n_u))
    u0 = 0.2 * kr.project(s.B, np.full(s.n_u, s.h ** s.dim), np.random.default_rng(2).standard_normal(s.n_u))[0]
    ns.gfu.data = hipla.Vector.from_numpy(u0)
    p0 = np.random.default_rng(4).standard_normal(s.n_p)
    ns.gfup.data = hipla.Vector.from_numpy(0.01 * (p0 - p0.mean()))
    if buoyant:
        ns.AddScalar(initial=np.random.default_rng(6).random(s.n_p), precision=1e-12, maxsteps=5000, kappa=0.8,
                     dirichlet=WALLS, buoyancy=beta, t_ref=0.5)
    if projection is not None:
        ns.SetProjection(projection)
    if implicit is not None:
        ns.SetImplicitSolve(implicit)
    if treatment is not None:
        ns.SetConvectionTreatment(treatment)
    return ns


def start_of(ns):
    sc = ns._scalar
    scalar = None if sc is None else dict(ops=sc.ops, T=ns.temperature.numpy().copy(), w_b=sc.w_b, t_ref=sc.t_ref)
    return ns.system, ns.gfu.numpy().copy(), ns.f.vec.numpy().copy(), scalar


def state(ns):
    out = [ns.gfu.numpy().copy(), ns.gfup.numpy().copy()]
    return out + ([ns.temperature.numpy().copy()] if ns._scalar is not None else [])


def assert_state(ns, ref, what):
    errs = [rel(ns.gfu.numpy(), ref["u"])]
    p, q = ns.gfup.numpy(), ref["phi"]
    errs.append(rel(p - p.mean(), q - q.mean()))
    if "T" in ref:
        errs.append(rel(ns.temperature.numpy(), ref["T"]))
    print("%s: relative differences (u, gfup, T) %s" % (what, ["%.3g" % e for e in errs]))
    assert max(errs) <= 1e-9, errs


def tighten(ns):
    ops = ns._time_stepping_operators()
    if ns.projection == "cg":
        ops["invproj"].precision, ops["invproj"].maxsteps = 1e-13, 20000
    inv = ns._implicit_momentum_solver(None)
    inv.precision, inv.maxsteps = 1e-12, 4000


CASES = [(grid, buoyant, mode, projection, implicit) for grid in sorted(GRIDS) for buoyant in (False, True)
         for mode in sorted(MODES) for projection in ("cg", "fdm") for implicit in ("cg", "fdm")]


@pytest.mark.parametrize("grid,buoyant,mode,projection,implicit", CASES)
def test_advance_against_the_reference_steps(hip_engine, grid, buoyant, mode, projection, implicit):
    ns = fresh(grid, buoyant, projection, implicit)
    s, u, f, scalar = start_of(ns)
    rec = ns.Advance(3, **MODES[mode](slice(0, 3)), **TIGHT)
    assert ns.advance_declined is None and rec.declined is None
    assert rec.convection_treatment == "implicit" and rec.implicit == implicit and rec.projection == projection
    assert rec.mstar_iterations.shape == (3,) and (rec.mstar_iterations > 0).all()
    assert (rec.scalar_iterations > 0).all() if buoyant else rec.scalar_iterations is None
    taus = [TAU] * 3 if mode == "fixed" else list(rec.timestep)
    if mode == "cfl":
        assert rec.cfl[0] == pytest.approx(4.0, rel=1e-12) and taus[0] > TAU      # a step the explicit scheme cannot take
    ref, energy = icr.reference_run(s, u, f, taus, scalar)
    assert_state(ns, ref, "%s buoyant=%s %s projection=%s implicit=%s, iterations %s"
                 % (grid, buoyant, mode, projection, implicit, rec.mstar_iterations))
    assert np.allclose(rec.kinetic_energy, energy, rtol=1e-9, atol=0.0)


@pytest.mark.parametrize("grid", sorted(GRIDS))
@pytest.mark.parametrize("buoyant", [False, True])
@pytest.mark.parametrize("implicit", ["cg", "fdm"])
def test_do_time_step_against_the_reference_steps(hip_engine, grid, buoyant, implicit):
    ns = fresh(grid, buoyant, "fdm", implicit)
    tighten(ns)
    s, u, f, scalar = start_of(ns)
    quiet(ns.DoTimeStep)
    quiet(ns.DoTimeStep, timestep=0.2)
    quiet(ns.DoTimeStep)
    inv = ns._last_momentum_solver
    assert inv._fused is not None and inv._fused.form is not None and inv.iterations > 0      # the device loop ran
    ref, _ = icr.reference_run(s, u, f, [TAU, 0.2, TAU], scalar)
    assert_state(ns, ref, "DoTimeStep %s buoyant=%s implicit=%s" % (grid, buoyant, implicit))


def test_the_stepper_holds_the_loop_and_no_cg(hip_engine):
    ns = fresh("3d", True, "fdm", "cg")
    ns.Advance(1)
    (stepper,) = ns._steppers.values()
    (scalar,) = ns._scalar.steppers.values()
    assert stepper.cg_m is None and stepper.mstar is None and stepper.bicg_m is not None and stepper.dinv_m is not None
    assert scalar.cg is None and scalar.mstar is None and scalar.bicg is not None
    assert stepper.bicg_m.mat is stepper.AD and scalar.bicg.mat is scalar.KB    # the stepper's own [A | D] and [K | B]


# ---- 4. bits --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["fixed", "timesteps"])
@pytest.mark.parametrize("implicit", ["cg", "fdm"])
def test_split_advance_is_bit_identical(hip_engine, mode, implicit):
    one, two = fresh("2d", True, "fdm", implicit), fresh("2d", True, "fdm", implicit)
    kw = MODES[mode]
    rec = one.Advance(4, **kw(slice(0, 4)))
    first, second = two.Advance(2, **kw(slice(0, 2))), two.Advance(2, **kw(slice(2, 4)))
    for a, b in zip(state(one), state(two)):
        assert np.array_equal(a, b)
    for name in ("div_norm", "kinetic_energy", "wall_flux", "mstar_iterations", "scalar_iterations"):
        assert np.array_equal(getattr(rec, name), np.concatenate([getattr(first, name), getattr(second, name)])), name


@pytest.mark.parametrize("grid", sorted(GRIDS))
def test_advance_against_do_time_step_repeated(hip_engine, grid):
    ns, twin = fresh(grid, True, "fdm", "cg"), fresh(grid, True, "fdm", "cg")
    tighten(twin)
    ns.Advance(3, **TIGHT)
    for _ in range(3):
        quiet(twin.DoTimeStep)
    errs = [rel(a, b) for a, b in zip(state(ns), state(twin))]
    print("Advance against DoTimeStep repeated (u, gfup, T): %s" % ["%.3g" % e for e in errs])
    assert max(errs) <= 1e-8


@pytest.mark.parametrize("buoyant", [False, True])
def test_an_object_back_at_explicit_keeps_the_default_bits(hip_engine, buoyant):
    def run(switch):
        ns = fresh("2d", buoyant, treatment=None)
        if switch:
            ns.SetConvectionTreatment("implicit")
            ns.SetConvectionTreatment("explicit")
        quiet(ns.DoTimeStep)
        quiet(ns.DoTimeStep, 0.03)
        recs = [ns.Advance(2), ns.Advance(2, timesteps=[0.02, 0.04])]
        assert all(r.convection_treatment == "explicit" for r in recs)
        assert set(ns._steppers) == {"jacobi", ("variable", "jacobi")}
        return state(ns) + [r.mstar_iterations for r in recs] + [r.kinetic_energy for r in recs]
    for a, b in zip(run(False), run(True)):
        assert np.array_equal(a, b)


def test_a_breakdown_puts_the_last_finished_step_back(hip_engine):
    """A force that is not finite makes the right-hand side of the velocity solve not finite: the loop reports code 1 at
    its start, `Advance` raises and `gfu` holds the state of the last finished step."""
    import hipla
    ns = fresh("2d")
    ns.Advance(2)
    before = state(ns)
    f = ns.f.vec.numpy().copy()
    f[3] = np.inf
    ns.f.vec.data = hipla.Vector.from_numpy(f)
    with pytest.raises(FloatingPointError, match="code 1"):
        ns.Advance(2)
    for a, b in zip(before, state(ns)):
        assert np.array_equal(a, b)
