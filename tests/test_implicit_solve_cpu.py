"""`hipla.stepping.ImplicitSolve.kind_of` and `check_implicit_solve` over the full product of their arguments, without
an engine: the kind against a table written out here, the refusals against the rules of the two steppers restated here
with the texts and in the order in which `TimeStepper.try_create` and `ScalarStepper` have always raised them."""

import itertools

from hipla.stepping import ImplicitSolve, check_implicit_solve

KINDS = {   # (variable, implicit, convection treatment) -> kind: implicit convection wins, then the direct solve
    (False, "cg", "explicit"): "cg",
    (False, "fdm", "explicit"): "fdm",
    (True, "cg", "explicit"): "shifted",
    (True, "fdm", "explicit"): "fdm",
    (False, "cg", "implicit"): "bicgstab",
    (False, "fdm", "implicit"): "bicgstab",
    (True, "cg", "implicit"): "bicgstab",
    (True, "fdm", "implicit"): "bicgstab",
}


def test_the_kind_of_every_combination_of_the_switches():
    product = set(itertools.product((False, True), ("cg", "fdm"), ("explicit", "implicit")))
    assert product == set(KINDS)
    for switches, kind in KINDS.items():
        assert ImplicitSolve.kind_of(*switches) == kind, switches


IMPLICIT_CONVECTION = "implicit convection goes with time_scheme=\"euler\", convection=\"upwind\" and inner_pre=\"jacobi\""
VARIABLE = "a variable-step stepper takes inner_pre=\"jacobi\""


def velocity_refusal(inner_pre, implicit, variable, time_scheme, convection, treatment, projection):
    """The message of `TimeStepper.try_create` (None: it goes on): no prefix; the names of `inner_pre` and `projection`
    are checked between the rule of implicit convection and the name of `implicit`."""
    direct = implicit == "fdm"
    if treatment == "implicit":
        if time_scheme != "euler" or convection != "upwind" or not (inner_pre == "jacobi" or direct):
            return IMPLICIT_CONVECTION
    if inner_pre != "jacobi" and inner_pre != "amg":
        return "inner_pre is \"jacobi\" or \"amg\""
    if projection != "cg" and projection != "fdm":
        return "projection is \"cg\" or \"fdm\""
    if implicit != "cg" and not direct:
        return "implicit is \"cg\" or \"fdm\""
    if variable and not direct and inner_pre != "jacobi":
        return VARIABLE + ": a hierarchy belongs to one step size"
    return None


def scalar_refusal(inner_pre, implicit, variable, time_scheme, convection, treatment):
    """The message of `ScalarStepper(...)`: its name in front, no check of the name of `inner_pre`, the short text for
    variable steps."""
    direct = implicit == "fdm"
    if treatment == "implicit":
        if time_scheme != "euler" or convection != "upwind" or not (inner_pre == "jacobi" or direct):
            return "ScalarStepper: " + IMPLICIT_CONVECTION
    if implicit != "cg" and not direct:
        return "ScalarStepper: implicit is \"cg\" or \"fdm\""
    if variable and not direct and inner_pre != "jacobi":
        return "ScalarStepper: " + VARIABLE
    return None


ARGUMENTS = list(itertools.product(("jacobi", "amg", "ilu"), ("cg", "fdm", "lu"), (False, True), ("euler", "cnab2"),
                                   ("upwind", "minmod", "vanleer"), ("explicit", "implicit")))


def outcome(*args, **kw):
    try:
        check_implicit_solve(*args, **kw)
    except ValueError as err:
        return str(err)
    return None


def test_the_velocity_stepper_refuses_what_it_always_refused():
    raised = 0
    for args in ARGUMENTS:
        for projection in ("cg", "fdm", "lu"):
            want = velocity_refusal(*args, projection)
            assert outcome("TimeStepper", *args, projection=projection) == want, (args, projection)
            raised += want is not None
        assert outcome("TimeStepper", *args) == velocity_refusal(*args, "cg"), args        # (the default projection)
    assert 0 < raised < 3 * len(ARGUMENTS)


def test_the_scalar_stepper_refuses_what_it_always_refused():
    raised = 0
    for args in ARGUMENTS:
        want = scalar_refusal(*args)
        assert outcome("ScalarStepper", *args) == want, args
        raised += want is not None
    assert 0 < raised < len(ARGUMENTS)

