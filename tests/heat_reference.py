"""Dense restatement of `heat.evolve` shared by the heat-integrator tests and the golden generator: the reference's
loop (heat.py:74-146) with ``scipy.sparse.linalg.splu`` for ``heat^-1``, a numpy modified Gram-Schmidt in the order of
orthonormalization.py:5-16 and the package's implicit Runge-Kutta step.  Results are computed once per case and shared
(callers must not modify them)."""

import functools

import numpy as np
import scipy.sparse as sp
from scipy.sparse.linalg import splu

KL = [(1, 1), (2, 1), (1, 3), (3, 3), (2, 3), (4, 5), (5, 2)]        # the reference's modes: seven distinct eigenvalues
END_TIME = 0.05
# time_step -> (steps, end time reached, the larger relative l2 error against the discrete exact solution), measured
# with the reference's own Runge-Kutta module and a numpy restatement of its loop at n = 16, 32, 64
ERROR_TABLE = {
    1e-1: (1, 0.1, 3.0e-2),
    10 ** -1.5: (2, 0.0632, 2.05e-4),
    1e-2: (5, 0.05, 8.7e-5),
    10 ** -2.5: (16, 0.0506, 5.4e-5),
    1e-3: (50, 0.05, 2.2e-6),
}
ERROR_FACTOR = 1.5          # guards only against another valid quadrature of the weights (the error is the method's)
RESTATEMENT_BOUND = 1e-8    # 1e4 x precision 1e-12: measured sensitivity to the inner solves <= 2.2e3 per unit


def numpy_mgs(columns, tries=3):
    """`columns`: list of 1-D arrays, orthonormalised in place in the reference's operation order; returns them."""
    for _ in range(tries):
        for j, bj in enumerate(columns):
            for bi in columns[:j]:
                bj -= (bi @ bj) / (bi @ bi) * bi
            bj *= 1 / np.sqrt(bj @ bj)
    return columns


def krylov_columns(temperature, K, m, time_step, dimension=5):
    """The un-orthonormalised basis of one step: [T] and dimension - 1 sub-steps (heat.py:87-98)."""
    lu = splu((sp.diags(m) + time_step * K).tocsc())
    dt = time_step / dimension
    temperature = temperature.copy()
    columns = [temperature.copy()]
    for _ in range(1, dimension):
        temperature -= dt * lu.solve(K @ temperature)
        columns.append(temperature.copy())
    return columns


def dense_evolve(initial_temperature, end_time, time_step, K, m, dimension=5, stages=10, trace=None):
    """Returns (temperature, time, steps).  `trace`: a list that receives the evolution matrix of every step."""
    from runge_kutta_method import ImplicitRungeKuttaMethodWeights, linear_implicit_runge_kutta_step
    K = sp.csr_matrix(K)
    lu = splu((sp.diags(m) + time_step * K).tocsc())
    weights = ImplicitRungeKuttaMethodWeights(stages)
    dt = time_step / dimension
    temperature = np.array(initial_temperature, dtype=np.float64)
    time, steps = 0, 0
    while time < end_time:
        time += time_step
        columns = [temperature.copy()]
        norm0 = np.sqrt(temperature @ temperature)
        for _ in range(1, dimension):
            temperature -= dt * lu.solve(K @ temperature)
            columns.append(temperature.copy())
        V = np.array(numpy_mgs(columns)).T
        evolution = -np.linalg.inv(V.T @ (m[:, None] * V)) @ (V.T @ (K @ V))
        if trace is not None:
            trace.append(evolution)
        y = np.zeros(dimension)
        y[0] = norm0
        temperature = V @ linear_implicit_runge_kutta_step(weights, evolution, y, time_step)
        steps += 1
    return temperature, time, steps


@functools.lru_cache(maxsize=None)
def restated(n, time_step, mass_seed=None):
    """(K, m, start, (temperature, time, steps)) of the dense restatement on the n x n grid from the reference's modes;
    `mass_seed`: a random lumped mass in [0.5, 2] instead of ones."""
    from heat import sum_of_unit_square_laplace_eigenfunctions
    from staggered_grid import diffusion_operators_2d
    K, m = diffusion_operators_2d(n)
    if mass_seed is not None:
        m = 0.5 + 1.5 * np.random.default_rng(mass_seed).random(n * n)
    start = sum_of_unit_square_laplace_eigenfunctions(KL, n)
    return K, m, start, dense_evolve(start, END_TIME, time_step, K, m)


def relative_l2(a, b):
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))
