"""Variable time steps on the product engine: the shifted operator of the fused CG (`EpiCgShiftQ`, csrc/cg.hip) and its
Jacobi kernel on their own, the CFL rate kernel (csrc/step.hip) against the numpy statement written in its order, and
`NavierStokes.Advance(timesteps=)` / `Advance(cfl=)` against tests/variable_step_reference.py (direct solves), against
the fixed-step `Advance`, against `DoTimeStep(timestep=)` and against itself across calls.

Tolerances.  The shifted operator, per row r of nnz_r entries: the fp64 result of m_r p_r + sigma (A p)_r -- nnz_r
products and nnz_r - 1 additions for the row, one product m_r p_r, one fma -- errs by at most
gamma_{nnz_r + 2} (|m_r p_r| + sigma (|A||p|)_r) whatever the order of the row's sum; the bound used is
(nnz_r + 3) 2^-53 of that scale.  The Jacobi kernel and the rate kernel are compared for equality.  `Advance`: 1e-13 /
1e-9 / 1e-8 for what stands in front of a solve, behind the velocity solve, and behind both converged solves
(DESIGN.md section 3), as in tests/test_cnab2_gpu.py."""

import contextlib
import io
from fractions import Fraction

import numpy as np
import pytest
import scipy.sparse as sp

from oracle import krylov_ref as kr
from test_step_kernels_gpu import LD, SENT, absvec, flag, matvec, ptr, refused
from variable_step_reference import VariableStepReference

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
TIGHT = dict(precision=1e-14, maxsteps=(5000, 20000))


def rel(a, b):
    nb = np.linalg.norm(b)
    return np.linalg.norm(np.asarray(a) - b) / nb if nb else float(np.linalg.norm(a))


def mean_free(p):
    return p - p.mean()


# ---- 1. the shifted operator ----------------------------------------------------------------------------------------
def banded_spd(n=300, seed=7):
    """Seeded SPD matrix with 40 entries in every row: offsets +-1 .. +-19 and n / 2 (wrapped), the diagonal dominant."""
    rng = np.random.default_rng(seed)
    mat = sp.lil_matrix((n, n))
    idx = np.arange(n)
    for k in range(1, 20):
        w = -rng.random(n)
        mat[idx, (idx + k) % n] = w
        mat[(idx + k) % n, idx] = w
    w = -rng.random(n // 2)
    mat[idx[:n // 2], idx[:n // 2] + n // 2] = w
    mat[idx[:n // 2] + n // 2, idx[:n // 2]] = w
    mat = mat.tocsr()
    mat.setdiag(np.asarray(abs(mat).sum(axis=1)).ravel() + 1.0 + rng.random(n))
    mat = mat.tocsr()
    mat.sort_indices()
    assert (np.diff(mat.indptr) == 40).all() and abs(mat - mat.T).max() == 0.0
    return mat


def shift_matrix(name):
    from staggered_grid import mac_stokes
    if name == "mac2d":
        mat = mac_stokes(2, 24, 0.01).A.tocsr()
        assert mat.shape[0] == 1104
    elif name == "mac3d":
        mat = mac_stokes(3, 6, 0.01).A.tocsr()
    elif name == "banded":
        mat = banded_spd()
    else:
        mat = sp.csr_matrix([[2.5]])
    mat.sort_indices()
    return mat


def shifted_loop(eng, mat, mass, storage):
    """(CgLoop with a shift over `mat`, the host matrix the device streams)."""
    import hipla
    from hipla import fused
    from hipla.matrix import fp32_copy, round32
    A = hipla.SparseMatrix.from_scipy(mat)
    host = mat
    if storage == "fp32":
        A, host = fp32_copy(A), round32(mat)
        assert hipla.matrix.value_bytes(A) == 4 * mat.nnz
    loop = fused.CgLoop(eng, A, fused.NO_PRE, shift=(mass, eng.from_host(host.diagonal())))
    return loop, host


def masses(n, kind, seed=11):
    return np.full(n, 0.37) if kind == "uniform" else 0.1 + np.random.default_rng(seed).random(n)


SHIFT_CASES = [(name, kind, storage) for name in ("mac2d", "mac3d", "banded", "one") for kind in ("vector", "uniform")
               for storage in ("fp64", "fp32")]


@pytest.mark.parametrize("name,kind,storage", SHIFT_CASES)
def test_shifted_operator_one_iteration(hip_engine, name, kind, storage):
    """After `nss_cg_start`, the q of iteration 0 is m p + sigma A p of the start direction p = dinv b, row by row within
    (nnz_r + 3) 2^-53 (|m_r p_r| + sigma (|A||p|)_r) of the long-double value; the Jacobi kernel's dinv equals
    1 / fma(sigma, d, m) bit for bit.  2-D n = 24: 1104 rows, several row blocks with a partial last one; rows of 40
    entries: off the row-per-lane path; one row; mass as a vector and as one value; fp64 and fp32 values."""
    import ctypes as C
    eng = hip_engine
    mat = shift_matrix(name)
    n = mat.shape[0]
    mass, sigma = masses(n, kind), 0.0371
    loop, host = shifted_loop(eng, mat, mass, storage)
    assert (loop.state.shift_mass is None) == (kind == "uniform" or n == 1)
    if name == "mac2d":
        assert len(loop.mat.handle.row_blocks()) - 1 > 2
    loop.set_shift(sigma)
    diag = host.diagonal()
    want_dinv = np.array([1.0 / float(Fraction(sigma) * Fraction(d) + Fraction(m)) for d, m in zip(diag, mass)])
    assert np.array_equal(eng.to_host(loop.pa.diag.d), want_dinv)
    b = np.random.default_rng(5).standard_normal(n)
    x = eng.from_host(np.full(n, 7.0))
    loop.hist = eng.zeros(4)
    loop.state.hist, loop.state.x = loop.hist.data_ptr(), x.data_ptr()
    d_b = eng.from_host(b)
    eng._check(eng.lib.nss_cg_start(C.byref(loop.state), d_b.data_ptr(), 1e-30, eng.stream))
    p = eng.to_host(loop.work["p"]).copy()
    assert np.array_equal(p, want_dinv * b)
    eng.upload(np.full(n, SENT), loop.work["q"])
    loop.enqueue(0, 1)
    q = eng.to_host(loop.work["q"])
    want = mass.astype(LD) * p.astype(LD) + LD(sigma) * matvec(host, p)
    scale = np.abs(mass * p) + sigma * absvec(host, p)
    err = np.abs(np.asarray(q.astype(LD) - want, dtype=np.float64))
    bound = (np.diff(host.indptr) + 3) * U * scale
    print("shifted q %s/%s/%s n=%d max err / bound = %.3f" % (name, kind, storage, n, float((err / bound).max())))
    assert (err <= bound).all(), (np.nonzero(err > bound)[0][:8], float((err / bound).max()))
    pq = float(eng.to_host(loop.scal)[1])
    assert abs(pq - float(np.dot(p.astype(LD), want))) <= (n + 43) * U * float(np.dot(np.abs(p), scale))


@pytest.mark.parametrize("name", ["mac2d", "banded", "one"])
def test_zero_sigma_is_the_plain_loop(hip_engine, name):
    """A state whose shift_sigma is 0 runs the loop as it was: the bits of the plain Jacobi-CG loop (x, history,
    count), with the shift's other fields set."""
    import hipla
    from hipla import fused
    eng = hip_engine
    mat = shift_matrix(name)
    n = mat.shape[0]
    A = hipla.SparseMatrix.from_scipy(mat)
    pre = hipla.JacobiPreconditioner(A)
    plain = fused.CgLoop.try_create(A, pre)
    loop, _ = shifted_loop(eng, mat, masses(n, "vector"), "fp64")
    loop.set_shift(0.5)
    loop.state.shift_sigma = 0.0
    eng.copy(plain.pa.diag.d, loop.pa.diag.d)
    b = eng.from_host(np.random.default_rng(6).standard_normal(n))
    x1, x2 = eng.zeros(n), eng.zeros(n)
    it1, it2 = plain.solve_resident(b, x1, 1e-12, 3000), loop.solve_resident(b, x2, 1e-12, 3000)
    assert it1 == it2 and 0 < it1 < 3000
    assert np.array_equal(eng.to_host(x1), eng.to_host(x2))
    assert np.array_equal(eng.to_host(plain.hist)[:it1], eng.to_host(loop.hist)[:it1])


@pytest.mark.parametrize("name,kind,storage", [c for c in SHIFT_CASES if c[0] != "mac3d" or c[2] == "fp64"])
def test_shifted_solves(hip_engine, name, kind, storage):
    """Full solves at precision 1e-14 for two sigmas through one loop: the iteration count is within one of the plain
    loop's on the assembled M + sigma A, the solutions agree to 1e-10."""
    import hipla
    from hipla import fused
    eng = hip_engine
    mat = shift_matrix(name)
    n = mat.shape[0]
    mass = masses(n, kind)
    loop, host = shifted_loop(eng, mat, mass, storage)
    b = eng.from_host(np.random.default_rng(9).standard_normal(n))
    for sigma in (0.05, 0.0125):
        full = hipla.SparseMatrix.from_scipy((sp.diags(mass) + sigma * host).tocsr())
        plain = fused.CgLoop.try_create(full, hipla.JacobiPreconditioner(full))
        x1, x2 = eng.zeros(n), eng.zeros(n)
        it1 = plain.solve_resident(b, x1, 1e-14, 5000)
        loop.set_shift(sigma)
        it2 = loop.solve_resident(b, x2, 1e-14, 5000)
        err = rel(eng.to_host(x2), eng.to_host(x1))
        print("shifted solve %s/%s/%s sigma=%g iterations %d / %d rel %.3e" % (name, kind, storage, sigma, it2, it1, err))
        assert abs(it1 - it2) <= 1 and 0 < it2 < 5000 and err < 1e-10


def test_shift_refusals(hip_engine):
    import hipla
    from hipla import fused
    from hipla.hip_engine import NssError
    eng = hip_engine
    mat = shift_matrix("mac3d")
    n = mat.shape[0]
    loop, _ = shifted_loop(eng, mat, masses(n, "vector"), "fp64")
    b, x = eng.from_host(np.ones(n)), eng.zeros(n)
    with pytest.raises(ValueError, match="set_shift"):
        loop.solve_resident(b, x, 1e-8, 10)                   # no sigma yet
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="sigma"):
            loop.set_shift(bad)
    with pytest.raises(ValueError, match="shift"):
        fused.CgLoop(eng, loop.mat, fused.NO_PRE, shift=(np.ones(n - 1), eng.zeros(n)))
    plain = fused.CgLoop.try_create(loop.mat, None)
    with pytest.raises(ValueError, match="without a shift"):
        plain.set_shift(0.1)
    A = hipla.SparseMatrix.from_scipy(mat)
    from staggered_grid import mac_stokes
    bj = fused.CgLoop.try_create(A, hipla.BlockJacobi(A, mac_stokes(3, 6, 0.01).line_blocks(3)))
    bj.state.shift_sigma = 0.1                                # a shifted state with block Jacobi: refused before a launch
    with pytest.raises(NssError, match="shifted loop"):
        bj.solve_resident(b, x, 1e-8, 10)
    assert eng.lib.nss_cg_shift_jacobi_f64(n, None, 1.0, 0.1, None, x.data_ptr(), eng.stream) != 0
    assert b"cg_shift_jacobi" in eng.lib.nss_last_error()


# ---- 2. the rate kernel ---------------------------------------------------------------------------------------------
def rate_host(b, u, w):
    """The statement of step_cfl_kernel in its order: rows summed entry after entry, products rounded on their own."""
    b = sp.csr_matrix(b)
    top = 0.0
    for r in range(b.shape[0]):
        total = 0.0
        for p in range(b.indptr[r], b.indptr[r + 1]):
            total += abs(float(b.data[p])) * abs(float(u[b.indices[p]]))
        v = float(w[r]) * total
        top = max(top, v if np.isfinite(v) else np.inf)
    return top


def rate_device(eng, Bm, u, w, done=None, slot=2, slots=4, cap=None):
    """One nss_step_cfl_f64 launch into out[slot] of `slots` sentinels; returns (rc, out, partials)."""
    import ctypes as C
    count = C.c_int64()
    eng._check(eng.lib.nss_step_cfl_workspace(Bm.handle.ptr, C.byref(count)))
    assert count.value == (Bm.height + 255) // 256 or Bm.height == 0
    part, out = eng.from_host(np.full(count.value + 2, SENT)), eng.from_host(np.full(slots, SENT))
    uniform = np.ndim(w) == 0
    d_w = None if uniform else eng.from_host(w)
    d_u = eng.from_host(u)
    rc = eng.lib.nss_step_cfl_f64(Bm.handle.ptr, d_u.data_ptr(), ptr(d_w), float(w) if uniform else 0.0,
                                  part.data_ptr(), count.value if cap is None else cap, out.data_ptr(), slot, ptr(done),
                                  eng.stream)
    return rc, eng.to_host(out), eng.to_host(part), count.value


def random_rows(rng, m=700, n=300):
    """Seeded CSR with 0 .. 9 entries per row, empty rows among them, the first and last rows not empty."""
    lens = rng.integers(0, 10, size=m)
    lens[[0, m - 1, 600]] = [3, 4, 5]
    lens[[1, 5, m - 2]] = 0
    rows = np.repeat(np.arange(m), lens)
    cols = np.concatenate([rng.choice(n, size=k, replace=False) for k in lens])
    return sp.csr_matrix((rng.standard_normal(rows.size), (rows, cols)), shape=(m, n))


def rate_inputs(name):
    from staggered_grid import mac_stokes
    rng = np.random.default_rng(17)
    if name == "random":
        b = random_rows(rng)
        return b, 0.5 + rng.random(b.shape[0])
    s = mac_stokes(2, 8, 0.01) if name == "mac2d" else mac_stokes(3, 5, 0.01)
    return s.B.tocsr(), 1.0 / s.h ** s.dim


@pytest.mark.parametrize("name", ["mac2d", "mac3d", "random"])
def test_rate_kernel_equals_the_host_statement(hip_engine, name):
    """out[slot] equals the numpy statement written in the kernel's order, bit for bit: a seeded u with negative
    entries; the maximum placed in the first row, the last row and the tail block; u = 0 gives 0; a NaN or an inf in u
    gives +inf; the other slots and the entries behind the partials are left alone."""
    import hipla
    eng = hip_engine
    b, w = rate_inputs(name)
    m, n = b.shape
    Bm = hipla.SparseMatrix.from_scipy(b)
    rng = np.random.default_rng(23)
    base = rng.standard_normal(n)
    assert (base < 0).any() and (b.data < 0).any()
    cases = [base]
    for row in (0, m - 1, m - 1 - (m % 256) // 2 if m > 256 else m // 2):     # first row, last row, inside the tail block
        u = base.copy()
        u[b.indices[b.indptr[row]:b.indptr[row + 1]]] *= 1e3
        cases.append(u)
    tops = []
    for k, u in enumerate(cases):
        rc, out, part, count = rate_device(eng, Bm, u, w)
        want = rate_host(b, u, np.full(m, w) if np.ndim(w) == 0 else w)
        assert rc == 0 and out[2] == want and want > 0, (k, out[2], want)
        assert (out[[0, 1, 3]] == SENT).all() and (part[count:] == SENT).all() and (part[:count] <= want).all()
        tops.append(want)
    if name != "random":                                   # on the plain grid: max_cell sum_faces |u_f| / h
        from staggered_grid import mac_stokes
        s = mac_stokes(2, 8, 0.01) if name == "mac2d" else mac_stokes(3, 5, 0.01)
        np.testing.assert_allclose(tops[0], (abs(s.B) @ np.abs(base)).max() / s.h ** s.dim, rtol=1e-14)
        vec = rate_device(eng, Bm, base, np.full(m, w))[1][2]                   # the weights as a vector: the same bits
        assert vec == tops[0]
    assert len(set(tops)) == 4                             # the placed maxima were the maxima
    assert rate_device(eng, Bm, np.zeros(n), w)[1][2] == 0.0
    col = int(b.indices[b.indptr[m - 1]])
    for poison in (np.nan, np.inf, -np.inf):
        u = base.copy()
        u[col] = poison
        assert rate_device(eng, Bm, u, w)[1][2] == np.inf, poison


def test_rate_kernel_done_cap_and_refusals(hip_engine):
    import hipla
    eng = hip_engine
    b, w = rate_inputs("random")
    Bm = hipla.SparseMatrix.from_scipy(b)
    u = np.random.default_rng(3).standard_normal(b.shape[1])
    rc, out, part, count = rate_device(eng, Bm, u, w, done=flag(eng, 1))
    assert rc == 0 and (out == SENT).all() and (part == SENT).all()                 # done: nothing written
    rc, out, part, count = rate_device(eng, Bm, u, w, done=flag(eng, 0))
    assert rc == 0 and out[2] == rate_host(b, u, w)
    rc, out, part, count = rate_device(eng, Bm, u, w, cap=count - 1)
    refused(eng, rc, "step_cfl")
    assert (out == SENT).all() and (part == SENT).all()                             # refused before any launch
    rc, out, part, count = rate_device(eng, Bm, u, w, slot=-1)
    refused(eng, rc, "step_cfl")
    assert eng.lib.nss_step_cfl_f64(None, None, None, 1.0, None, 0, None, 0, None, eng.stream) != 0
    assert eng.lib.nss_step_cfl_workspace(None, None) != 0
    narrow = hipla.matrix.fp32_copy(Bm)
    rc = rate_device(eng, narrow, u, w)[0]
    refused(eng, rc, "step_cfl")


# ---- 3. Advance -----------------------------------------------------------------------------------------------------
TAU = 0.05
WALLS = {"x-": 1.0, "x+": 0.0}
GRIDS = {"2d": (2, 8, (0.0, 2.0)), "3d": (3, 5, (0.0, 2.0, -1.0))}


def scalar_args(grid):
    return dict(kappa=0.8, dirichlet=WALLS, buoyancy=GRIDS[grid][2], t_ref=0.5)


def fresh(grid, convection="vanleer", buoyant=True, time_scheme="cnab2"):
    """`fresh` of tests/test_cnab2_gpu.py: converged inner solvers in the statements (here also invmstar), a seeded
    divergence-free start (max |u| tau / h about 0.1), a seeded force and start pressure, optionally a buoyant scalar."""
    import hipla
    from templates.NavierStokesSIMPLE_iterative import NavierStokes, SyntheticMesh
    dim, n, _ = GRIDS[grid]
    ns = NavierStokes(SyntheticMesh(1.0 / n, dim=dim), nu=0.01, inflow="inlet", outflow="outlet", wall="wall|cyl",
                      uin=None, timestep=TAU, order=0, convection=convection, time_scheme=time_scheme)
    s = ns.system
    assert s.block_size == 1 and s.n == n
    ns.f.vec.data = hipla.Vector.from_numpy(0.5 * s.h ** s.dim * np.random.default_rng(8).standard_normal(s.n_u))
    u0 = 0.2 * kr.project(s.B, np.full(s.n_u, s.h ** s.dim), np.random.default_rng(2).standard_normal(s.n_u))[0]
    ns.gfu.data = hipla.Vector.from_numpy(u0)
    p0 = np.random.default_rng(4).standard_normal(s.n_p)
    ns.gfup.data = hipla.Vector.from_numpy(0.01 * (p0 - p0.mean()))
    if buoyant:
        ns.AddScalar(initial=np.random.default_rng(6).random(s.n_p), precision=1e-14, maxsteps=5000, **scalar_args(grid))
    ops = ns._time_stepping_operators()
    ops["invmstar"] = hipla.CGSolver(ops["mstar"], pre=hipla.JacobiPreconditioner(ops["mstar"]), precision=1e-14, maxsteps=5000)
    ops["invproj"] = hipla.CGSolver(ops["Lp"], pre=hipla.JacobiPreconditioner(ops["Lp"]), precision=1e-14, maxsteps=20000)
    if time_scheme == "cnab2":
        half = ns._cnab2_operators()
        half["invmhalf"] = hipla.CGSolver(half["mhalf"], pre=hipla.JacobiPreconditioner(half["mhalf"]), precision=1e-14,
                                          maxsteps=5000)
    return ns


def reference_of(ns, grid, buoyant):
    sc = dict(scalar_args(grid), convection=ns._scalar.convection) if buoyant else None
    return VariableStepReference(ns.system, ns.timestep, ns.gfu.numpy(), ns.f.vec.numpy(), ns.convection, ns.time_scheme,
                                 scalar=sc, T0=ns.temperature.numpy() if buoyant else None, q0=ns.gfup.numpy())


def state(ns, buoyant=True):
    out = [ns.gfu.numpy(), mean_free(ns.gfup.numpy())] + ([ns.temperature.numpy()] if buoyant else [])
    if ns.time_scheme == "cnab2":
        out += [ns.F_prev.numpy()] + ([ns.G_prev.numpy(), ns.b_prev.numpy()] if buoyant else [])
    return out


def raw_state(ns, buoyant=True):
    return state(ns, buoyant) + [ns.gfup.numpy()]


def statement_steps(ns, sizes):
    with contextlib.redirect_stdout(io.StringIO()):
        for tau in sizes:
            ns.DoTimeStep(timestep=tau)


def stage_errors(eng, ns, want, buoyant):
    st = ns._steppers[("variable", "jacobi")]
    cnab2 = ns.time_scheme == "cnab2"
    errs = dict(F_ext=rel(eng.to_host(st.F), want["F_ext"]), temp=rel(eng.to_host(st.temp), want["temp"]),
                raw=rel(eng.to_host(st.raw), want["raw"]), temp2=rel(eng.to_host(st.temp2), want["temp2"]),
                u=rel(ns.gfu.numpy(), want["u"]), q=rel(mean_free(ns.gfup.numpy()), mean_free(want["q"])))
    if cnab2:
        errs.update(F_prev=rel(ns.F_prev.numpy(), want["F"]))
    if buoyant:
        ss = ns._scalar.steppers["variable"]
        errs.update(G_ext=rel(eng.to_host(ss.G), want["G_ext"]), f_step=rel(eng.to_host(ss.f_eff), want["f_step"]),
                    temp_T=rel(eng.to_host(ss.temp), want["temp_T"]), delta=rel(eng.to_host(ss.delta), want["delta"]),
                    T=rel(ns.temperature.numpy(), want["T"]))
        if cnab2:
            errs.update(G_prev=rel(ns.G_prev.numpy(), want["G"]), b_prev=rel(ns.b_prev.numpy(), want["b"]))
    return errs


@pytest.mark.parametrize("buoyant", [False, True])
@pytest.mark.parametrize("scheme", ["euler", "cnab2"])
@pytest.mark.parametrize("grid", ["2d", "3d"])
def test_prescribed_steps_against_the_reference(hip_engine, grid, scheme, buoyant):
    """`Advance(2, timesteps=[0.05, 0.03])` with converged inner solves against the reference's `step_with`, the stages
    of its second step (weights (1 + r/2, -r/2), r = 0.6, sigma of the shifted solves from 0.03) to 1e-8; and on a twin
    `Advance(1, timesteps=[0.03])`, a first step of another size than the object's, at the tight bounds: 1e-13 in front
    of the solves, 1e-9 for raw and delta, 1e-8 behind.  The record holds the sizes, their sum and tau_n rate(u^n)."""
    eng = hip_engine
    ns, twin = fresh(grid, buoyant=buoyant, time_scheme=scheme), fresh(grid, buoyant=buoyant, time_scheme=scheme)
    ref, ref_twin = reference_of(ns, grid, buoyant), reference_of(twin, grid, buoyant)
    rates = [ref.rate()]
    ref.step_with(0.05)
    rates.append(ref.rate())
    want = ref.step_with(0.03)
    rec = ns.Advance(2, timesteps=[0.05, 0.03], **TIGHT)
    assert rec.declined is None and ns.advance_declined is None and rec.time_scheme == scheme
    assert ("variable", "jacobi") in ns._steppers and "jacobi" not in ns._steppers
    st = ns._steppers[("variable", "jacobi")]
    assert st.mstar is None and st.cg_m.mat is ns.a.mat and st.cg_m.sigma == (0.015 if scheme == "cnab2" else 0.03)
    assert not buoyant or ns._scalar.steppers["variable"].mstar is None
    errs = stage_errors(eng, ns, want, buoyant)
    print(grid, scheme, buoyant, "second step", errs, rec.mstar_iterations, rec.proj_iterations)
    assert max(errs.values()) < 1e-8, errs
    assert np.array_equal(rec.timestep, [0.05, 0.03]) and np.array_equal(rec.time, np.cumsum([0.05, 0.03]))
    np.testing.assert_allclose(rec.cfl, np.array(rates) * [0.05, 0.03], rtol=1e-8)
    assert rec.limited_by is None and ns._clock.tau_prev == 0.03
    assert abs(rec.div_norm[1] - np.linalg.norm(ns.system.B @ ns.gfu.numpy())) <= 1e-9 * np.linalg.norm(ns.gfu.numpy())
    want = ref_twin.step_with(0.03)
    twin.Advance(1, timesteps=[0.03], **TIGHT)
    errs = stage_errors(eng, twin, want, buoyant)
    print(grid, scheme, buoyant, "first step", errs)
    for key, err in errs.items():
        bound = 1e-8 if key in ("temp2", "u", "q", "T") else 1e-9 if key in ("raw", "delta") else 1e-13
        assert err < bound, (key, err, bound)


@pytest.mark.parametrize("scheme", ["euler", "cnab2"])
def test_equal_prescribed_steps_against_the_fixed_step(hip_engine, scheme):
    """`timesteps=[TAU] * 5` against the fixed `Advance(5)`: the same scheme through the shifted loops -- u, q, T and the
    histories to 1e-8, the iteration counts within one."""
    ns, fixed = fresh("2d", time_scheme=scheme), fresh("2d", time_scheme=scheme)
    rec, rec_fixed = ns.Advance(5, timesteps=[TAU] * 5, **TIGHT), fixed.Advance(5, **TIGHT)
    errs = [rel(a, b) for a, b in zip(state(ns), state(fixed))]
    print(scheme, errs, rec.mstar_iterations, rec_fixed.mstar_iterations)
    assert max(errs) < 1e-8, errs
    assert np.abs(rec.mstar_iterations - rec_fixed.mstar_iterations).max() <= 1
    assert rec_fixed.timestep is None and rec_fixed.cfl is None and fixed._clock.tau_prev == TAU


SIZES = [0.05, 0.03, 0.04, 0.02, 0.045]


@pytest.mark.parametrize("scheme", ["euler", "cnab2"])
@pytest.mark.parametrize("mode", ["timesteps", "cfl"])
def test_split_variable_advance_is_bit_identical(hip_engine, scheme, mode):
    """`Advance(timesteps=t[:2])` followed by `Advance(timesteps=t[2:])` has the bits of `Advance(timesteps=t)`: the
    history, q and the size of the last step are handed over exactly.  The same for `cfl=` split 2 + 3 (the growth
    limit reads the last step of the earlier call)."""
    one, two = fresh("2d", time_scheme=scheme), fresh("2d", time_scheme=scheme)
    if mode == "timesteps":
        one.Advance(5, timesteps=SIZES, **TIGHT)
        two.Advance(2, timesteps=SIZES[:2], **TIGHT)
        two.Advance(3, timesteps=SIZES[2:], **TIGHT)
    else:
        kw = dict(cfl=0.05, max_timestep=0.08, growth=1.5, **TIGHT)
        for ns in (one, two):                   # a small step first: the growth limit then binds for four steps (the rate
            ns.Advance(1, timesteps=[0.001], **TIGHT)      # of the start field is 7.9, cfl / rate = 0.0063)
        rec = one.Advance(5, **kw)
        a, b = two.Advance(2, **kw), two.Advance(3, **kw)
        assert np.array_equal(rec.timestep, np.concatenate([a.timestep, b.timestep]))
        assert rec.limited_by == a.limited_by + b.limited_by == ["growth"] * 4 + ["cfl"]
        assert b.timestep[0] == 1.5 * a.timestep[1]        # the growth limit read the last step of the earlier call
    for x, y in zip(raw_state(one), raw_state(two)):
        assert np.array_equal(x, y)
    assert one._clock.tau_prev == two._clock.tau_prev


@pytest.mark.parametrize("scheme", ["euler", "cnab2"])
@pytest.mark.parametrize("grid", ["2d", "3d"])
def test_statements_then_variable_advance(hip_engine, grid, scheme):
    """Two `DoTimeStep(timestep=)` followed by a variable `Advance(3)` against five statement steps: u, q, T and the
    histories to 1e-8; then a fixed `Advance(1)` on both (r = TAU / 0.045 through the object's history)."""
    mixed, twin = fresh(grid, time_scheme=scheme), fresh(grid, time_scheme=scheme)
    statement_steps(mixed, SIZES[:2])
    rec = mixed.Advance(3, timesteps=SIZES[2:], **TIGHT)
    statement_steps(twin, SIZES)
    assert rec.declined is None
    errs = [rel(a, b) for a, b in zip(state(mixed), state(twin))]
    print(grid, scheme, errs)
    assert max(errs) < 1e-8, errs
    mixed.Advance(1, **TIGHT)
    statement_steps(twin, [None])
    assert max(rel(a, b) for a, b in zip(state(mixed), state(twin))) < 1e-8
    assert mixed._clock.tau_prev == twin._clock.tau_prev == TAU


@pytest.fixture(scope="module")
def controller_reference():
    """The CPU controller case (tests/test_variable_step_cpu.py): 2-D n = 8, nu = 0.05, smooth start with peak 1,
    cfl = 0.4, max_timestep = 0.05 -- the reference's runs for growth 1.25 (24 steps) and 1.1 (16 steps), once."""
    from test_variable_step_cpu import CONTROLLED, controller_case
    s, u0, f = controller_case()
    return {growth: VariableStepReference(s, 0.05, u0, f, *CONTROLLED).run_controlled(nsteps, 0.4, 0.05, growth)
            for growth, nsteps in ((1.25, 24), (1.1, 16))}


@pytest.mark.parametrize("growth,nsteps", [(1.25, 24), (1.1, 16)])
def test_controller_on_the_device(hip_engine, controller_reference, growth, nsteps):
    """The `cfl=` run of the CPU controller case through the device-resident stepper: the reference's step sizes to 1e-9
    relative, its codes exactly, every cfl[k] within the target, `CflRate()` = the host value."""
    from test_variable_step_cpu import controlled_product
    taus, codes, numbers = controller_reference[growth]
    ns = controlled_product()
    u0 = ns.gfu.numpy()
    host_rate = float(((abs(ns.system.B) @ np.abs(u0)) / ns.system.mass).max())
    assert abs(ns.CflRate() - host_rate) <= 1e-14 * host_rate and abs(host_rate - 16.0) <= 16e-14
    rec = ns.Advance(nsteps, cfl=0.4, growth=growth, **TIGHT)
    assert rec.declined is None and rec.limited_by == codes
    assert (np.abs(rec.timestep / taus - 1) <= 1e-9).all(), np.abs(rec.timestep / taus - 1).max()
    assert (rec.cfl <= 0.4 * (1 + 1e-12)).all() and np.allclose(rec.cfl, numbers, rtol=1e-8)
    assert np.array_equal(rec.time, np.cumsum(rec.timestep)) and ns._clock.tau_prev == rec.timestep[-1]


def test_duration_and_non_finite_rate_on_the_device(hip_engine):
    import hipla
    from test_variable_step_cpu import controlled_product
    ns = controlled_product()
    rec = ns.Advance(40, cfl=0.4, duration=0.33, **TIGHT)
    assert rec.declined is None and rec.limited_by[-1] == "end" and rec.limited_by.count("end") == 1
    assert abs(rec.time[-1] - 0.33) <= 1e-14 * 0.33 and len(rec.timestep) == len(rec.mstar_iterations) < 40
    assert len(rec.div_norm) == len(rec.timestep)
    bad = controlled_product()
    u = bad.gfu.numpy().copy()
    u[3] = np.nan
    bad.gfu.data = hipla.Vector.from_numpy(u)
    assert bad.CflRate() == np.inf
    with pytest.raises(FloatingPointError):
        bad.Advance(2, cfl=0.4)
    assert np.array_equal(bad.gfu.numpy(), u, equal_nan=True) and bad._clock.tau_prev is None


def test_amg_and_pseudo_raise(hip_engine):
    ns = fresh("2d", buoyant=False)
    for kw in (dict(timesteps=[0.01, 0.02], inner_pre="amg"), dict(cfl=0.4, inner_pre="amg"),
               dict(timesteps=[0.01, 0.02], pseudo=True), dict(timesteps=[0.01, 0.02], cfl=0.4), dict(timesteps=[0.01]),
               dict(timesteps=[0.01, 0.0]), dict(growth=1.5), dict(cfl=0.4, growth=0.5)):
        with pytest.raises(ValueError):
            ns.Advance(2, **kw)
    assert not getattr(ns, "_steppers", {})


@pytest.mark.parametrize("scheme", ["euler", "cnab2"])
def test_declined_flux_kernel_with_variable_steps(hip_engine, scheme):
    """Convection operators the flux kernel refuses (recorded as refused in the object's shared dict, as in
    tests/test_cnab2_gpu.py): a "cnab2" object declines the device step as for fixed steps and runs the statements -- the
    bits of `DoTimeStep(timestep=)`; an "euler" stepper keeps running on the device with the protocol's convection
    operator and records `flux_declined`."""
    ns, twin = fresh("2d", time_scheme=scheme), fresh("2d", time_scheme=scheme)
    ops = ns._time_stepping_operators()
    why = "adv: a row holds 3 entries (the row-per-lane kernels take two)"
    ns._stepper_shared = dict(mstar=ops["mstar"], Lp=ops["Lp"], C=ops["correct"], flux_declined=why)
    if scheme == "cnab2":
        ns._stepper_shared["mhalf"] = ns._cnab2_operators()["mhalf"]
    rec = ns.Advance(2, timesteps=[0.05, 0.03], **TIGHT)
    statement_steps(twin, [0.05, 0.03])
    if scheme == "cnab2":
        assert rec.declined == ns.advance_declined and "cnab2" in rec.declined and why in rec.declined
        for a, b in zip(raw_state(ns), raw_state(twin)):
            assert np.array_equal(a, b)
    else:
        assert rec.declined is None and rec.flux_declined == why
        assert max(rel(a, b) for a, b in zip(state(ns), state(twin))) < 1e-8
    assert np.array_equal(rec.timestep, [0.05, 0.03]) and len(rec.mstar_iterations) == 2
