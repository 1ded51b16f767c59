"""`heat.evolve` on the CPU checker engine (its protocol path: no HIP engine) against the dense restatement of
tests/heat_reference.py and against the discrete exact solution, with the reference's seven modes.

Bounds (tests/heat_reference.py): the error against the exact solution is the method's -- at most 1.5 x the larger value
measured with the reference's own Runge-Kutta module for that step size; against the restatement 1e4 x the inner
solves' precision 1e-12 (a relative perturbation eps of every inner solve moves the result by at most 2.2e3 eps,
measured at n = 16 and 33)."""

import numpy as np
import pytest
import scipy.sparse as sp

import heat_reference as hr


@pytest.mark.parametrize("time_step", sorted(hr.ERROR_TABLE, reverse=True))
def test_error_table(numpy_engine, time_step):
    import heat
    steps, end, bound = hr.ERROR_TABLE[time_step]
    n = 16
    start = heat.sum_of_unit_square_laplace_eigenfunctions(hr.KL, n)
    temperature, time, record = heat.evolve(start, hr.END_TIME, time_step, n=n)
    assert record.steps == steps and record.cg_iterations.shape == (steps, 4)
    assert abs(time - steps * time_step) <= 1e-12 and abs(time - end) <= 5e-5
    assert record.declined is not None
    error = hr.relative_l2(temperature, heat.exact_solution(hr.KL, time, n))
    print("time_step %.3e: %d steps, error %.3e" % (time_step, steps, error))
    assert error <= hr.ERROR_FACTOR * bound


@pytest.mark.parametrize("n", [32, 64])
def test_error_hardly_depends_on_n(numpy_engine, n):
    import heat
    time_step = 10 ** -1.5
    steps, _, bound = hr.ERROR_TABLE[time_step]
    temperature, time, record = heat.evolve(heat.sum_of_unit_square_laplace_eigenfunctions(hr.KL, n), hr.END_TIME,
                                            time_step, n=n)
    assert record.steps == steps
    assert hr.relative_l2(temperature, heat.exact_solution(hr.KL, time, n)) <= hr.ERROR_FACTOR * bound


@pytest.mark.parametrize("n", [16, 33])
@pytest.mark.parametrize("time_step", [1e-2, 10 ** -1.5])
def test_decline_path_agrees_with_the_dense_restatement(numpy_engine, n, time_step):
    import heat
    K, m, start, (ref, ref_time, ref_steps) = hr.restated(n, time_step)
    temperature, time, record = heat.evolve(start, hr.END_TIME, time_step, n=n, diagnostics=True)
    assert (time, record.steps) == (ref_time, ref_steps)
    assert record.declined == "not the HIP engine"
    difference = hr.relative_l2(temperature, ref)
    print("n %d time_step %.3e: difference %.3e, |V^T V - I| %.1e" % (n, time_step, difference,
                                                                    record.orthogonality.max()))
    assert difference <= hr.RESTATEMENT_BOUND
    assert record.orthogonality.max() <= 5e-14
    assert (record.cg_iterations > 0).all() and (record.cg_iterations < 10 * n).all()


def test_non_uniform_mass_through_operators(numpy_engine):
    import heat
    n, time_step = 16, 1e-2
    K, m, start, (ref, ref_time, ref_steps) = hr.restated(n, time_step, mass_seed=5)
    assert m.min() >= 0.5 and m.max() <= 2.0 and m.std() > 0.1
    temperature, time, record = heat.evolve(start, hr.END_TIME, time_step, operators=(K, m))
    assert record.steps == ref_steps
    assert hr.relative_l2(temperature, ref) <= hr.RESTATEMENT_BOUND


def test_exact_solution_is_exact_for_the_grid_operator():
    import heat
    from staggered_grid import diffusion_operators_2d
    n = 9
    K, m = diffusion_operators_2d(n)
    h = 1.0 / (n + 1)
    for k, l in hr.KL:
        mode = heat.sum_of_unit_square_laplace_eigenfunctions([(k, l)], n)
        lam = (4 / h ** 2) * (np.sin(k * np.pi * h / 2) ** 2 + np.sin(l * np.pi * h / 2) ** 2)
        assert np.abs(K @ mode - lam * mode).max() <= 1e-12 * lam * np.abs(mode).max()
        assert np.abs(heat.exact_solution([(k, l)], 0.01, n) - np.exp(-0.01 * lam) * mode).max() <= 1e-14
    x = np.arange(1, n + 1) * h                                   # x is the fastest index
    assert np.allclose(heat.sum_of_unit_square_laplace_eigenfunctions([(2, 1)], n).reshape(n, n)[3],
                       2 * np.sin(2 * np.pi * x) * np.sin(np.pi * x[3]), rtol=0, atol=1e-15)
    assert np.array_equal(heat.exact_solution(hr.KL, 0.0, n), heat.sum_of_unit_square_laplace_eigenfunctions(hr.KL, n))


@pytest.mark.parametrize("n, dt", [(1, 0.5), (7, 1e-3), (16, 10 ** -1.5)])
def test_diffusion_2d_is_mass_plus_dt_diffusion(n, dt):
    from staggered_grid import diffusion_2d, diffusion_operators_2d
    K, m = diffusion_operators_2d(n)
    assert m.shape == (n * n,) and (m == 1).all() and K.shape == (n * n, n * n)
    whole, parts = diffusion_2d(n, dt), (sp.diags(m) + dt * K).tocsr()
    parts.sort_indices()
    assert np.array_equal(whole.indptr, parts.indptr) and np.array_equal(whole.indices, parts.indices)
    assert np.array_equal(whole.data, parts.data)                 # exactly


def test_rank_deficient_start_raises_value_error(numpy_engine):
    """A single mode is an eigenvector: every sub-step vector is a multiple of it.  On the 1 x 1 grid that is exact in
    floating point (the second column projects to 0.0); on larger grids the rounding of K T leaves a column of noise,
    which the orthonormalisation normalises -- a valid basis, not an error.  A zero start divides 0 by 0."""
    import heat
    single = heat.sum_of_unit_square_laplace_eigenfunctions([(1, 1)], 1)
    with pytest.raises(ValueError, match="step 0"):
        heat.evolve(single, hr.END_TIME, 1e-2, n=1)
    with pytest.raises(ValueError, match="step 0"):
        heat.evolve(np.zeros(16), hr.END_TIME, 1e-2, n=4)
    temperature, _, _ = heat.evolve(heat.sum_of_unit_square_laplace_eigenfunctions([(1, 1)], 8), 0.02, 1e-2, n=8)
    assert np.isfinite(temperature).all()
    assert hr.relative_l2(temperature, heat.exact_solution([(1, 1)], 0.02, 8)) <= 1e-9
