"""BASELINE.json config 1 ("heat.py 2D diffusion, 64x64 grid, CG") and the heat exponential integrator.

`conjugate_gradients`, `krylov_galerkin` and `solve` drive the plumbing operations the reference's heat.py performs on
single (non-block) vectors -- SpMV (heat.py:96,110,116), AXPY (:97,140-142), InnerProduct / Norm (:89,112,117) and the
Gram-Schmidt of orthonormalization.py -- through the protocol on the 5-point ``M + dt*K`` matrix of
`staggered_grid.diffusion_2d`.

`evolve` is the integrator itself (heat.py:74-146): per time step a 5-dimensional Krylov basis from implicit sub-steps,
its orthonormalisation, the Galerkin matrices of diffusion and mass, and one Gauss-Legendre implicit Runge-Kutta step
of the small system (`runge_kutta_method`) -- on the 5-point grid operators of `staggered_grid.diffusion_operators_2d`
instead of the reference's order-10 H1 space, and with the fused CG in place of its sparse direct inverse."""

from math import sqrt

import numpy as np

import hipla
from hipla import InnerProduct, Norm
from orthonormalization import orthonormalize
from runge_kutta_method import ImplicitRungeKuttaMethodWeights, linear_implicit_runge_kutta_step
from staggered_grid import diffusion_2d, diffusion_operators_2d


def conjugate_gradients(mat, rhs, tol=1e-10, maxsteps=1000):
    """Textbook CG on ``mat * x = rhs`` with protocol operations only; returns (x, history) with
    history[i] = sqrt(<r_i, r_i>)."""
    x, r, p, q = (rhs.CreateVector() for _ in range(4))
    x[:] = 0.0
    r.data = rhs
    p.data = r
    rz = InnerProduct(r, r)
    history = [sqrt(rz)]
    for _ in range(maxsteps):
        q.data = mat * p
        alpha = rz / InnerProduct(p, q)
        x.data += alpha * p
        r.data -= alpha * q
        rz_new = InnerProduct(r, r)
        history.append(sqrt(rz_new))
        if history[-1] < tol * history[0]:
            break
        p.data = r + (rz_new / rz) * p
        rz = rz_new
    return x, history


def conjugate_gradients_fused(mat, rhs, tol=1e-10, maxsteps=1000):
    """The same CG through `hipla.CGSolver` (device-resident loop ``nss_cg_*`` on the GPU)."""
    solver = hipla.CGSolver(mat, pre=None, precision=tol, maxsteps=maxsteps)
    x = rhs.CreateVector()
    x.data = solver * rhs
    return x, solver.errors


def krylov_galerkin(mat, start, dimension=5):
    """Krylov basis {v, Mv, .., M^(d-1) v}, orthonormalised (heat.py:95-100), and its Galerkin
    matrix G[r, c] = <b_r, M b_c> (heat.py:109-118)."""
    basis = [start.Copy()]
    for _ in range(1, dimension):
        nxt = basis[-1].CreateVector()
        nxt.data = mat * basis[-1]
        basis.append(nxt)
    basis = orthonormalize(basis)
    galerkin = np.zeros((dimension, dimension))
    residual = start.CreateVector()
    for col in range(dimension):
        residual.data = mat * basis[col]
        for row in range(dimension):
            galerkin[row, col] = InnerProduct(basis[row], residual)
    return basis, galerkin


def solve(n=64, dt=1e-3, seed=3, tol=1e-10):
    """Config-1 run: returns (x, cg_history, galerkin_matrix) for the n x n diffusion matrix."""
    mat = hipla.SparseMatrix.from_scipy(diffusion_2d(n, dt))
    rhs = hipla.Vector.from_numpy(np.random.default_rng(seed).standard_normal(n * n))
    x, history = conjugate_gradients(mat, rhs, tol=tol)
    _, galerkin = krylov_galerkin(mat, rhs)
    return x, history, galerkin


def _grid_modes(kl, n, decay):
    x = np.arange(1, n + 1) / (n + 1)
    h = 1.0 / (n + 1)
    out = np.zeros((n, n))
    for k, l in kl:
        lam = (4.0 / (h * h)) * (np.sin(k * np.pi * h / 2) ** 2 + np.sin(l * np.pi * h / 2) ** 2)
        out += 2 * decay(lam) * np.outer(np.sin(l * np.pi * x), np.sin(k * np.pi * x))
    return out.reshape(-1)


def sum_of_unit_square_laplace_eigenfunctions(kl, n):
    """``sum_{(k, l)} 2 sin(k pi x) sin(l pi y)`` at the n x n interior grid points (x fastest), heat.py:13-18."""
    return _grid_modes(kl, n, lambda lam: 1.0)


def exact_solution(kl, t, n):
    """The DISCRETE exact solution at time `t` from `sum_of_unit_square_laplace_eigenfunctions(kl, n)` (heat.py:21-27):
    the modes are exact eigenvectors of the 5-point operator of `diffusion_operators_2d` with
    ``lambda = (4 / h^2) (sin^2(k pi h / 2) + sin^2(l pi h / 2))``, so mode (k, l) decays by ``exp(-lambda t)``."""
    return _grid_modes(kl, n, lambda lam: np.exp(-lam * t))


def _rank_deficient(step):
    return ValueError("heat.evolve: step %d: the Krylov basis is zero or rank-deficient (a vector of norm 0 or a "
                      "non-finite norm in the orthonormalisation)" % step)


def _subspace_step(step, norms, sub_diffusion, sub_mass, initial_norm, weights, time_step):
    """The small system of one step (heat.py:120-138): the coefficients of the next temperature in the basis.  `norms`:
    what the orthonormalisation divided by (any shape), checked here, once per step."""
    norms = np.asarray(norms, dtype=np.float64)
    if not (np.all(np.isfinite(norms)) and np.all(norms > 0.0) and np.all(np.isfinite(sub_diffusion))
            and np.all(np.isfinite(sub_mass))):
        raise _rank_deficient(step)
    evolution_matrix = -np.linalg.inv(sub_mass) @ sub_diffusion
    subspace_temperature = np.zeros(sub_mass.shape[0])
    subspace_temperature[0] = initial_norm
    return linear_implicit_runge_kutta_step(weights, evolution_matrix, subspace_temperature, time_step)


def evolve(initial_temperature, end_time, time_step, n=64, subspace_dimension=5, stages=10, precision=1e-12,
           maxsteps=None, inner_pre="jacobi", operators=None, diagnostics=False, on_step=None):
    """The reference's exponential integrator (heat.py:74-146), statement by statement: ``dt = time_step /
    subspace_dimension``; ``while time < end_time: time += time_step`` (the floating-point accumulation as written: it
    decides the number of steps); the basis ``[T]`` and `subspace_dimension` - 1 sub-steps ``T -= dt heat^-1 (K T)`` with
    ``heat = M + time_step K``; `orthonormalize`; ``Sd = V^T K V``, ``Sm = V^T M V``; ``E = -Sm^-1 Sd``, ``y = (|T_0|, 0,
    ..)``, one `linear_implicit_runge_kutta_step` with ``ImplicitRungeKuttaMethodWeights(stages)``; ``T = sum y_i V_i``.

    The one deliberate substitution: ``heat^-1`` is the fused preconditioned CG (`precision`, `maxsteps`; `inner_pre`:
    "jacobi" | "amg") instead of the reference's sparse direct inverse.

    `initial_temperature`: host array of length n^2 (`sum_of_unit_square_laplace_eigenfunctions`); `operators`:
    ``(K, m)`` -- a scipy matrix and a lumped mass diagonal -- instead of `diffusion_operators_2d(n)` (another grid, a
    non-uniform mass).  `diagnostics`: also record the largest entry of |V^T V - I| per step; `on_step(step)`: called
    after every step.  Returns ``(temperature, time, record)`` with a `hipla.stepping.HeatRecord`: on the HIP engine the
    step runs device-resident (`hipla.stepping.HeatIntegrator`); otherwise (no HIP engine, ``hipla.fused.ENABLED`` off) the
    same statements run through the protocol and ``record.declined`` says why.  A zero or rank-deficient basis raises
    `ValueError` naming the step."""
    import scipy.sparse as sp
    from hipla.stepping import HeatIntegrator, HeatRecord
    from hipla.matrix import JacobiPreconditioner
    if inner_pre not in ("jacobi", "amg"):
        raise ValueError("inner_pre is \"jacobi\" or \"amg\"")
    K, m = diffusion_operators_2d(n) if operators is None else operators
    K = sp.csr_matrix(K)
    m = np.asarray(m, dtype=np.float64)
    size = K.shape[0]
    start = np.asarray(initial_temperature, dtype=np.float64).reshape(-1)
    if start.size != size or m.size != size:
        raise ValueError("evolve: the temperature, the mass diagonal and K differ in size")
    d = int(subspace_dimension)
    maxsteps = max(200, 10 * int(np.sqrt(size))) if maxsteps is None else int(maxsteps)
    diffusion = hipla.SparseMatrix.from_scipy(K)
    mass = hipla.SparseMatrix.from_scipy(sp.diags(m, format="csr"))
    heat = hipla.SparseMatrix.from_scipy((sp.diags(m) + time_step * K).tocsr())
    pre = hipla.SmoothedAggregationAMG(heat) if inner_pre == "amg" else JacobiPreconditioner(heat)
    dt = time_step / d
    weights = ImplicitRungeKuttaMethodWeights(stages)
    iterations, orthogonality = [], [] if diagnostics else None
    time, step = 0, 0

    integrator = HeatIntegrator.try_create(diffusion, mass, heat, pre, d, diagnostics)
    if integrator is not None:
        integrator.load(start)
        while time < end_time:
            time += time_step
            its, norms, sub_diffusion, sub_mass, gram = integrator.build_subspace(dt, precision, maxsteps)
            next_temperature = _subspace_step(step, norms, sub_diffusion, sub_mass, sqrt(norms[0, 0]), weights,
                                              time_step)
            integrator.combine(next_temperature)
            iterations.append(its)
            if diagnostics:
                orthogonality.append(np.abs(gram - np.eye(d)).max())
            if on_step is not None:
                on_step(step)
            step += 1
        return integrator.temperature(), time, HeatRecord(iterations, orthogonality)

    declined = HeatIntegrator.last_declined
    heat_inverse = hipla.CGSolver(heat, pre=pre, precision=precision, maxsteps=maxsteps)
    temperature = hipla.Vector.from_numpy(start)
    residual, solution = temperature.CreateVector(), temperature.CreateVector()
    while time < end_time:
        time += time_step
        subspace_basis = [temperature.Copy()]
        initial_condition_norm = Norm(temperature)
        its = []
        for _ in range(1, d):
            residual.data = diffusion * temperature
            solution.data = heat_inverse * residual
            temperature.data -= dt * solution
            its.append(heat_inverse.iterations)
            subspace_basis.append(temperature.Copy())
        try:
            subspace_basis = orthonormalize(subspace_basis)
        except ZeroDivisionError:
            raise _rank_deficient(step) from None
        sub_diffusion, sub_mass, gram = np.zeros((d, d)), np.zeros((d, d)), np.zeros((d, d))
        for col in range(d):
            residual.data = diffusion * subspace_basis[col]
            for row in range(d):
                sub_diffusion[row, col] = InnerProduct(subspace_basis[row], residual)
            residual.data = mass * subspace_basis[col]
            for row in range(d):
                sub_mass[row, col] = InnerProduct(subspace_basis[row], residual)
            if diagnostics:
                for row in range(d):
                    gram[row, col] = InnerProduct(subspace_basis[row], subspace_basis[col])
        norms = [initial_condition_norm] + [InnerProduct(b, b) for b in subspace_basis]
        next_temperature = _subspace_step(step, norms, sub_diffusion, sub_mass, initial_condition_norm, weights,
                                          time_step)
        temperature[:] = 0
        for i, basis_vector in enumerate(subspace_basis):
            temperature.data += float(next_temperature[i]) * basis_vector
        iterations.append(its)
        if diagnostics:
            orthogonality.append(np.abs(gram - np.eye(d)).max())
        if on_step is not None:
            on_step(step)
        step += 1
    return temperature.numpy().copy(), time, HeatRecord(iterations, orthogonality, declined=declined)


if __name__ == "__main__":
    x, hist, gal = solve()
    print("CG iterations:", len(hist) - 1, " final residual:", hist[-1], " |x| =", Norm(x))
