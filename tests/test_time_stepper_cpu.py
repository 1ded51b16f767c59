"""Host side of the device-resident time stepping (no GPU): the C ABI of csrc/step.hip, the pseudo-inverse the AMG
applies on the coarsest level of a singular Laplacian, the two-entries-per-row detection, and `Advance`'s decline path on
the CPU checker engine."""

import contextlib
import io
import os
import subprocess

import numpy as np
import pytest
import scipy.sparse as sp

from conftest import ROOT

STEP_SYMBOLS = ("nss_step_flux_f64", "nss_step_rhs_f64", "nss_step_project_f64", "nss_step_divergence_f64",
                "nss_step_workspace", "nss_step_record_f64", "nss_cg_start")


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as entry
    from hipla.hip_engine import LIB_PATH, load_library
    if not os.path.exists(LIB_PATH):
        entry.build()
    return load_library()


def test_header_declares_the_step_entry_points():
    from test_cabi_symbols import declared_symbols
    names = declared_symbols()
    for must in STEP_SYMBOLS:
        assert must in names, must


def test_library_exports_the_step_entry_points(lib):
    from hipla.hip_engine import LIB_PATH, _signatures
    assert lib.nss_abi_version() == 1
    dynamic = subprocess.run(["nm", "-D", "--defined-only", LIB_PATH], check=True, capture_output=True, text=True).stdout
    exported = {line.split()[-1] for line in dynamic.splitlines() if line.strip()}
    for must in STEP_SYMBOLS:
        assert hasattr(lib, must) and must in exported and must in _signatures(), must


def test_step_entry_points_report_argument_errors(lib):
    assert lib.nss_step_flux_f64(None, None, None, None, None, None, None) != 0 and b"step_flux" in lib.nss_last_error()
    assert lib.nss_step_rhs_f64(None, None, None, None, None, None) != 0 and b"step_rhs" in lib.nss_last_error()
    assert lib.nss_step_project_f64(None, None, None, None, None, 0.0, None, None, 0, None, None) != 0
    assert lib.nss_step_divergence_f64(None, None, None, 0, None, None) != 0
    assert lib.nss_step_workspace(None, None, None, None) != 0
    assert lib.nss_step_record_f64(None, 0, None, 0, 1.0, None, 0, None, None) != 0
    assert lib.nss_cg_start(None, None, 1e-8, None) != 0 and b"cg" in lib.nss_last_error()


def neumann_laplacian(n):
    """5-point Laplacian of an n x n grid with no Dirichlet boundary: symmetric, kernel = constants."""
    t = sp.diags([-1.0, 2.0, -1.0], [-1, 0, 1], shape=(n, n)).tolil()
    t[0, 0] = t[n - 1, n - 1] = 1.0
    t = t.tocsr()
    return (sp.kron(sp.identity(n), t) + sp.kron(t, sp.identity(n))).tocsr()


def test_constants_pseudo_inverse():
    from hipla.amg import constants_pseudo_inverse
    fine = neumann_laplacian(6)
    agg = (np.arange(36) // 6 // 2) * 3 + (np.arange(36) % 6) // 2          # 2 x 2 aggregates
    tent = sp.csr_matrix((np.ones(36), (np.arange(36), agg)), shape=(36, 9))
    prol = tent - (2.0 / 3.0) * (sp.diags(1.0 / fine.diagonal()) @ fine @ tent)   # the smoothed prolongator
    coarse = (prol.T @ fine @ prol).toarray()
    for lap in (fine.toarray(), coarse):
        n = lap.shape[0]
        ones = np.ones(n)
        assert np.linalg.norm(lap @ ones) <= 1e-12 * abs(lap).sum()          # singular: the constants
        x = constants_pseudo_inverse(lap)
        assert np.abs(lap @ x @ lap - lap).max() <= 1e-10 * np.abs(lap).max()
        assert np.abs(x @ ones).max() <= 1e-10 * np.abs(x).max()
        assert np.array_equal(x, x.T)
        rhs = lap @ np.random.default_rng(0).standard_normal(n)               # consistent right-hand side
        assert np.linalg.norm(lap @ (x @ rhs) - rhs) <= 1e-10 * np.linalg.norm(rhs)


def test_two_entry_row_detection():
    from hipla.fused import constants_in_kernel, two_entry_rows
    from staggered_grid import mac_stokes
    for s in (mac_stokes(2, 6), mac_stokes(3, 5), mac_stokes(2, 5).inflate(3), mac_stokes(3, 4).inflate(3)):
        ops = s.convection_operators()
        for key in ("adv", "avg", "diff"):
            assert two_entry_rows(ops[key]) == (True, None), key
        bt = (sp.diags(np.full(s.n_u, s.h ** -s.dim)) @ s.B.T).tocsr()
        assert two_entry_rows(bt) == (True, None)                            # C = M_u^-1 B^T of the projection tail
        assert constants_in_kernel((s.B @ bt).tocsr())                       # the all-wall cavity
        ok, why = two_entry_rows(ops["div"])
        assert not ok and "entries" in why
    wide = sp.csr_matrix(np.array([[1.0, 0.0, 2.0, 0.0], [1.0, 1.0, 1.0, 0.0], [0.0, 0.0, 0.0, 0.0]]))
    ok, why = two_entry_rows(wide)
    assert not ok and "3 entries" in why
    assert two_entry_rows(sp.csr_matrix((0, 4))) == (True, None)
    assert not constants_in_kernel(sp.identity(4, format="csr"))


SUM_LENGTHS = (0, 1, 63, 64, 65, 1023, 1024, 1025, 4095, 4096, 4097, 8193, 35000)


@pytest.mark.parametrize("n", SUM_LENGTHS)
def test_fixed_tree_restatement_against_fsum(n):
    """oracle `fixed_sums_1024` -- the restatement of the device's summation tree that tests/test_step_kernels_gpu.py
    compares bit for bit -- is a sum: against math.fsum to 1e-13 * sum |x| (the tree is at most 25 additions deep:
    25 * 2^-53 = 3e-15), signed and non-negative terms, on both sides of every change of shape (one wave, one term
    per lane, four per lane: the strided loop's first trip, a second trip, many)."""
    from math import fsum
    from oracle import krylov_ref as kr
    rng = np.random.default_rng(100 + n)
    x, y = rng.standard_normal(n), rng.random(n)
    sx, sy = kr.fixed_sums_1024(x, y)
    assert abs(sx - fsum(x)) <= 1e-13 * fsum(np.abs(x))
    assert abs(sy - fsum(y)) <= 1e-13 * fsum(y)
    assert kr.fixed_sums_1024(y, x) == (sy, sx)
    assert (sy > 0.0) if n else (sx, sy) == (0.0, 0.0)
    ints = np.arange(1, n + 1, dtype=np.float64)                  # exact in every order: n (n + 1) / 2
    assert kr.fixed_sum_1024(ints) == n * (n + 1) / 2


def test_advance_declines_on_the_checker_engine(numpy_engine):
    """Not the HIP engine: Advance runs DoTimeStep / the pseudo-time statements, reports why, and gives their results."""
    import hipla
    from templates.NavierStokesSIMPLE_iterative import NavierStokes, SyntheticMesh

    def fresh():
        ns = NavierStokes(SyntheticMesh(0.2, dim=2), nu=0.01, inflow="inlet", outflow="outlet", wall="wall|cyl", uin=None,
                          timestep=0.05, order=1)
        ns.AddForce(np.random.default_rng(8).standard_normal(ns.system.n_u))
        ns.gfu.data = hipla.Vector.from_numpy(np.random.default_rng(2).standard_normal(ns.system.n_u))
        return ns

    ns, twin = fresh(), fresh()
    rec = ns.Advance(2)
    with contextlib.redirect_stdout(io.StringIO()):
        twin.DoTimeStep()
        twin.DoTimeStep()
    assert rec.declined == "not the HIP engine" == ns.advance_declined
    assert np.array_equal(ns.gfu.numpy(), twin.gfu.numpy())
    s, u = ns.system, ns.gfu.numpy()
    assert len(rec.mstar_iterations) == len(rec.proj_iterations) == 2 and (rec.proj_iterations > 0).all()
    assert abs(rec.div_norm[-1] - np.linalg.norm(s.B @ u)) <= 1e-9 * np.linalg.norm(s.B @ u)
    assert abs(rec.kinetic_energy[-1] - 0.5 * s.h ** s.dim * (u @ u)) <= 1e-12 * (u @ u)
    ops = ns._time_stepping_operators()
    assert (ops["invmstar"].precision, ops["invproj"].precision) == (1e-4, 1e-8)     # restored

    ns, twin = fresh(), fresh()
    rec = ns.Advance(2, pseudo=True, diagnostics=False)
    with contextlib.redirect_stdout(io.StringIO()):
        twin.SolveInitial(timesteps=2)
    assert rec.declined and rec.div_norm is None and rec.kinetic_energy is None
    assert np.array_equal(ns.gfu.numpy(), twin.gfu.numpy())
    with pytest.raises(ValueError):
        ns.Advance(1, inner_pre="ilu")


# ---- Advance(0) on the decline path: the contracts of tests/test_time_stepper_gpu.py without a device ----------------
def declined_case(scalar=None):
    """`scalar`: None, "wall" (a buoyant scalar whose Dirichlet wall is recorded) or "no wall" (buoyant, insulated)."""
    import hipla
    from templates.NavierStokesSIMPLE_iterative import NavierStokes, SyntheticMesh
    ns = NavierStokes(SyntheticMesh(0.2, dim=2), nu=0.01, inflow="inlet", outflow="outlet", wall="wall|cyl", uin=None,
                      timestep=0.05, order=0)
    s = ns.system
    ns.AddForce(0.1 * np.random.default_rng(8).standard_normal(s.n_u))
    ns.gfu.data = hipla.Vector.from_numpy(0.1 * np.random.default_rng(2).standard_normal(s.n_u))
    ns.gfup.data = hipla.Vector.from_numpy(np.random.default_rng(11).standard_normal(s.n_p))
    if scalar is not None:
        ns.AddScalar(0.8, dirichlet={"x-": 1.0, "x+": 0.0} if scalar == "wall" else None, buoyancy=(0.0, 40.0), t_ref=0.5,
                     initial=np.random.default_rng(6).random(s.n_p))
    return ns


@pytest.mark.parametrize("scalar,diagnostics", [(None, True), (None, False), ("wall", True), ("wall", False),
                                                ("no wall", True)])
def test_advance_zero_steps_by_statements(numpy_engine, scalar, diagnostics):
    """Advance(0) through `_advance_by_statements`: gfu, gfup and the temperature bit-unchanged; the record's arrays
    empty with the dtypes of Advance(1); None for the diagnostics without `diagnostics`, for the scalar's arrays without
    a scalar and for wall_flux without a flux wall."""
    ns = declined_case(scalar)
    u0, p0 = ns.gfu.numpy().copy(), ns.gfup.numpy().copy()
    T0 = None if scalar is None else ns.temperature.numpy().copy()
    rec = ns.Advance(0, diagnostics=diagnostics)
    assert rec.declined == "not the HIP engine"
    assert np.array_equal(ns.gfu.numpy(), u0) and np.array_equal(ns.gfup.numpy(), p0)
    assert scalar is None or np.array_equal(ns.temperature.numpy(), T0)
    one = ns.Advance(1, diagnostics=diagnostics)
    for name in ("mstar_iterations", "proj_iterations", "div_norm", "kinetic_energy", "scalar_iterations", "wall_flux"):
        got, ref = getattr(rec, name), getattr(one, name)
        if ref is None:
            assert got is None, name
        else:
            assert isinstance(got, np.ndarray) and got.shape == (0,) and got.dtype == ref.dtype and ref.shape == (1,), name
    assert (one.div_norm is None) == (one.kinetic_energy is None) == (not diagnostics)
    assert (one.scalar_iterations is None) == (scalar is None)
    assert (one.wall_flux is None) == (scalar != "wall" or not diagnostics)


def test_advance_zero_pseudo_steps_project_by_statements(numpy_engine):
    """Advance(0, pseudo=True) on the decline path is the leading Project(gfu): gfu agrees with `Project` on a twin to
    1e-8 (the bound of the device test), gfup is written, the record is empty."""
    ns, twin = declined_case(), declined_case()
    v0, p0 = ns.gfu.numpy().copy(), ns.gfup.numpy().copy()
    rec = ns.Advance(0, pseudo=True)
    twin.Project(twin.gfu)
    assert rec.declined == "not the HIP engine"
    assert np.linalg.norm(ns.gfu.numpy() - twin.gfu.numpy()) < 1e-8 * np.linalg.norm(twin.gfu.numpy())
    assert np.linalg.norm(ns.gfu.numpy() - v0) > 1e-2 * np.linalg.norm(v0)         # (the projection moved the field)
    assert not np.array_equal(ns.gfup.numpy(), p0) and np.isfinite(ns.gfup.numpy()).all()
    assert len(rec.mstar_iterations) == len(rec.proj_iterations) == len(rec.div_norm) == len(rec.kinetic_energy) == 0
    with pytest.raises(ValueError):
        declined_case("wall").Advance(0, pseudo=True)
