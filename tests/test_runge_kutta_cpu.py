"""`runge_kutta_method` (host, numpy) against the reference's module (tests/golden/heat_irk.npz, written by
tests/golden/make_golden_heat.py) and against what Gauss-Legendre collocation is known to be."""

import numpy as np
import pytest

from conftest import golden_path


@pytest.fixture(scope="module")
def golden():
    return np.load(golden_path("heat_irk"))


@pytest.mark.parametrize("deg", [1, 2, 3, 10])
def test_weights_against_the_reference(golden, deg):
    from runge_kutta_method import ImplicitRungeKuttaMethodWeights
    w = ImplicitRungeKuttaMethodWeights(deg)
    for name in ("a", "b", "c"):
        assert np.abs(getattr(w, name) - golden["%s_%d" % (name, deg)]).max() <= 1e-13, name


def test_steps_against_the_reference(golden):
    from runge_kutta_method import ImplicitRungeKuttaMethodWeights, linear_implicit_runge_kutta_step
    sizes = set()
    for i in range(int(golden["ncases"])):
        w = ImplicitRungeKuttaMethodWeights(int(golden["deg_%d" % i]))
        got = linear_implicit_runge_kutta_step(w, golden["matrix_%d" % i], golden["value_%d" % i],
                                               float(golden["width_%d" % i]))
        ref = golden["next_%d" % i]
        assert np.linalg.norm(got - ref) <= 1e-12 * np.linalg.norm(ref), i
        sizes.add(len(ref))
    assert sizes == {1, 3, 5}


@pytest.mark.parametrize("deg", [1, 2, 3, 5, 10])
def test_weights_are_gauss_legendre(deg):
    from runge_kutta_method import ImplicitRungeKuttaMethodWeights, lagrange
    w = ImplicitRungeKuttaMethodWeights(deg)
    nodes, gauss = np.polynomial.legendre.leggauss(deg)
    assert abs(w.b.sum() - 1) <= 1e-14
    assert np.abs(w.c - (nodes + 1) / 2).max() <= 1e-15            # the shifted Gauss nodes
    assert np.abs(w.b - gauss / 2).max() <= 1e-14
    assert np.abs(w.a.sum(axis=1) - w.c).max() <= 1e-14            # sum_j l_j = 1
    for j in range(deg):
        assert np.abs(lagrange(w.c, j, w.c) - np.eye(deg)[j]).max() <= 1e-12
    if deg == 3:
        assert np.abs(w.b - [5 / 18, 4 / 9, 5 / 18]).max() <= 1e-15
        assert np.abs(w.c - [0.5 - np.sqrt(15) / 10, 0.5, 0.5 + np.sqrt(15) / 10]).max() <= 1e-15


def scalar_step(deg, z):
    from runge_kutta_method import ImplicitRungeKuttaMethodWeights, linear_implicit_runge_kutta_step
    return linear_implicit_runge_kutta_step(ImplicitRungeKuttaMethodWeights(deg), np.array([[z]]), np.array([1.0]), 1.0)[0]


def test_one_stage_is_the_implicit_midpoint_rule():
    for z in (-3.0, -0.5, -1e-3, 0.25):
        assert abs(scalar_step(1, z) - (1 + z / 2) / (1 - z / 2)) <= 1e-15 * max(1.0, abs(z))


@pytest.mark.parametrize("deg", [1, 2, 3])
def test_scalar_step_has_order_2s(deg):
    """The stability function is the (s, s) Pade approximant of exp: its error is C z^(2s+1) (1 + O(z)) with
    C = s!^2 / ((2s)! (2s+1)!), so halving z divides the error by 2^(2s+1)."""
    from math import factorial
    errors = [abs(scalar_step(deg, z) - np.exp(z)) for z in (-0.4, -0.2)]
    constant = factorial(deg) ** 2 / (factorial(2 * deg) * factorial(2 * deg + 1))
    assert errors[1] <= 1.5 * constant * 0.2 ** (2 * deg + 1)
    assert 0.7 * 2 ** (2 * deg + 1) <= errors[0] / errors[1] <= 1.3 * 2 ** (2 * deg + 1)


def test_ten_stages_reproduce_exp_to_rounding():
    for z in (-2.0, -0.3, -1e-2):
        assert abs(scalar_step(10, z) - np.exp(z)) <= 1e-14
