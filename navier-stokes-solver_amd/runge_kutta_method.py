"""Gauss-Legendre implicit Runge-Kutta for linear systems y' = M y, with the reference's three names and meanings
(runge_kutta_method.py:6-59): `lagrange`, `ImplicitRungeKuttaMethodWeights`, `linear_implicit_runge_kutta_step`.

Host code on plain numpy arrays: the systems are the d x d evolution matrices of the heat integrator (`heat.evolve`).
Where the reference integrates the Lagrange polynomials by adaptive quadrature, the integrals here are exact: a
polynomial of degree deg - 1 over [0, c_i] by the deg-point Gauss rule mapped to that interval."""

import numpy as np


def lagrange(c, n, x):
    """The n-th Lagrange polynomial of the nodes `c` at `x`, ``prod_{m != n} (c_m - x) / (c_m - c_n)``; `x` may be an
    array (the result has its shape)."""
    c = np.asarray(c, dtype=np.float64).reshape(-1)
    x = np.asarray(x, dtype=np.float64)
    others = np.concatenate([c[:n], c[n + 1:]])
    return np.prod(others.reshape((-1,) + (1,) * x.ndim) - x, axis=0) / np.prod(others - c[n])


class ImplicitRungeKuttaMethodWeights:
    """Collocation at the `deg` Gauss-Legendre nodes of [0, 1]: ``c`` the nodes, ``b[i]`` the integral of the i-th
    Lagrange polynomial over [0, 1], ``a[i, j]`` that of the j-th over [0, c_i] (order 2 deg)."""

    def __init__(self, deg=3):
        nodes, weights = np.polynomial.legendre.leggauss(deg)
        self.c = (nodes + 1) / 2
        unit_nodes, unit_weights = (nodes + 1) / 2, weights / 2          # the same rule on [0, 1]
        self.a = np.zeros((deg, deg))
        self.b = np.zeros(deg)
        for j in range(deg):
            self.b[j] = unit_weights @ lagrange(self.c, j, unit_nodes)
            for i in range(deg):
                self.a[i, j] = self.c[i] * (unit_weights @ lagrange(self.c, j, self.c[i] * unit_nodes))


def linear_implicit_runge_kutta_step(weights, matrix, current_value, step_width):
    """One step of y' = matrix y: the stages solve ``(I - h a (x) M) k = 1 (x) (M y)``; returns ``y + h sum_i b_i k_i``."""
    matrix = np.atleast_2d(np.asarray(matrix, dtype=np.float64))
    current_value = np.asarray(current_value, dtype=np.float64).reshape(-1)
    a, b = np.asarray(weights.a, dtype=np.float64), np.asarray(weights.b, dtype=np.float64)
    stages, size = a.shape[0], matrix.shape[0]
    coefficient_matrix = np.eye(stages * size) - step_width * np.kron(a, matrix)
    inhomogeneity = np.tile(matrix @ current_value, stages)
    k = np.linalg.solve(coefficient_matrix, inhomogeneity).reshape(stages, size)
    return current_value + step_width * (b @ k)
