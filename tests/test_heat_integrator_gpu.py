"""`heat.evolve` on the HIP engine: the device-resident step (`hipla.fused.HeatIntegrator`) against the dense
restatement and the discrete exact solution (bounds: tests/heat_reference.py), its host traffic and its allocations."""

import numpy as np
import pytest

import heat_reference as hr

pytestmark = pytest.mark.gpu

MAXSTEPS = 400


@pytest.mark.parametrize("n", [16, 33])
@pytest.mark.parametrize("time_step", [1e-2, 10 ** -1.5])
def test_evolve_on_the_device(hip_engine, n, time_step):
    import heat
    torch = hip_engine.torch
    K, m, start, (ref, ref_time, ref_steps) = hr.restated(n, time_step)
    steps, _, bound = hr.ERROR_TABLE[time_step]
    allocated = []
    temperature, time, record = heat.evolve(start, hr.END_TIME, time_step, n=n, maxsteps=MAXSTEPS, diagnostics=True,
                                            on_step=lambda step: allocated.append(torch.cuda.memory_allocated()))
    assert record.declined is None
    assert record.steps == steps == ref_steps and time == ref_time
    difference = hr.relative_l2(temperature, ref)
    error = hr.relative_l2(temperature, heat.exact_solution(hr.KL, time, n))
    print("n %d time_step %.3e: difference %.3e, error %.3e, |V^T V - I| %.1e, CG %d .. %d"
          % (n, time_step, difference, error, record.orthogonality.max(), record.cg_iterations.min(),
             record.cg_iterations.max()))
    assert difference <= hr.RESTATEMENT_BOUND
    assert error <= hr.ERROR_FACTOR * bound
    assert record.orthogonality.max() <= 1e-14 * 5
    assert record.cg_iterations.shape == (steps, 4)
    assert (record.cg_iterations > 0).all() and (record.cg_iterations < MAXSTEPS).all()
    assert len(allocated) == steps and max(allocated[1:]) <= allocated[1]     # no growth from the second step on


def test_decline_path_on_the_device_engine(hip_engine):
    """`hipla.fused.ENABLED` off: the same statements through the protocol, on the same engine."""
    import heat
    from hipla import fused
    n, time_step = 16, 1e-2
    K, m, start, (ref, ref_time, ref_steps) = hr.restated(n, time_step)
    fused.ENABLED = False
    try:
        temperature, time, record = heat.evolve(start, hr.END_TIME, time_step, n=n, maxsteps=MAXSTEPS)
    finally:
        fused.ENABLED = True
    assert record.declined == "fused loops disabled (hipla.fused.ENABLED)"
    assert (time, record.steps) == (ref_time, ref_steps)
    assert hr.relative_l2(temperature, ref) <= hr.RESTATEMENT_BOUND


def test_non_uniform_lumped_mass(hip_engine):
    import heat
    n, time_step = 16, 1e-2
    K, m, start, (ref, ref_time, ref_steps) = hr.restated(n, time_step, mass_seed=5)
    temperature, time, record = heat.evolve(start, hr.END_TIME, time_step, operators=(K, m), maxsteps=MAXSTEPS)
    assert record.declined is None and record.steps == ref_steps
    difference = hr.relative_l2(temperature, ref)
    print("non-uniform mass: difference %.3e" % difference)
    assert difference <= hr.RESTATEMENT_BOUND


def test_rank_deficient_start_raises_value_error(hip_engine):
    import heat
    with pytest.raises(ValueError, match="step 0"):
        heat.evolve(heat.sum_of_unit_square_laplace_eigenfunctions([(1, 1)], 1), hr.END_TIME, 1e-2, n=1)
    with pytest.raises(ValueError, match="step 0"):
        heat.evolve(np.zeros(16), hr.END_TIME, 1e-2, n=4)
