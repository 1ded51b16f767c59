"""The joint AMG cycle of the auxiliary-space term (csrc/amg.hip: cycle_multi, csr_multi_kernel<K, L, Epi, VT>,
amg_diag_multi_kernel, multi_desc_kernel) at every branch of the kernel, on hand-made hierarchies (amg_cycle_cases.py),
against the long-double statement of the cycle (amg_cycle_reference.py): componentwise, |got_i - ref_i| <= tolerance * E_i
with the derived tolerance 2 * 2^-53 * sum over the kernels of (longest row + 3).  The same hierarchies go through the
single-vector kernels (amg_batch = 0, the plain handle) under the joint cycle's row-block plan.

Every case first proves from the handles' own row blocks that it contains the situation it is named for."""
import numpy as np
import pytest

import amg_cycle_cases as cases
import amg_cycle_reference as ref

pytestmark = pytest.mark.gpu

SCALES = (1.0, -1.5)


def _matrix_at(levels, where):
    return levels[-1]["inv"] if where == "inv" else levels[where[0]][where[1]]


def _operators(levels):
    return [lv[key] for lv in levels for key in ("A", "P", "R", "inv") if key in lv and not (key == "A" and "inv" in lv)]


def _generations(levels):
    return [m.handle.plan_generation() for m in _operators(levels)]


def _check_aux(engine, aux, name, K, storage, n_out, what, seed=11):
    worst = 0.0
    for bscale in SCALES:
        want, bound, tol = cases.auxiliary_reference(name, K, storage, bscale, seed)
        got = cases.apply(engine, aux, bscale, cases.right_hand_side(n_out, seed), n_out)
        worst = max(worst, ref.check(got, want, bound, tol, "%s K=%d %s %s bscale=%g" % (name, K, storage, what, bscale)))
    print("%s K=%d %s %s: |err_i| / (tolerance * E_i) <= %.3g" % (name, K, storage, what, worst))


@pytest.mark.parametrize("storage", ["fp64", "fp32"])
@pytest.mark.parametrize("K", [2, 3])
@pytest.mark.parametrize("name", cases.NAMES)
def test_joint_cycle_against_long_double(hip_engine, name, K, storage):
    eng = hip_engine
    case = cases.hierarchy(name)
    applied, _ = cases.engine_levels(case, eng, storage)
    plain = eng.amg_create(applied, case.omega)
    b0 = cases.right_hand_side(case.n0, 12)
    before = [cases.apply(eng, plain, s, b0, case.n0) for s in SCALES]
    gen0 = _generations(applied)
    T, TT = cases.engine_transform(name, K, eng, storage)
    n_out = T.height
    aux = eng.amg_create_auxiliary(T.handle, TT.handle, [plain] * K)
    assert all(g1 > g0 for g0, g1 in zip(gen0, _generations(applied))), "the shared hierarchy was not re-planned"
    if storage == "fp32":
        assert all(m.handle.value_bytes() == 4 * m.nnz for m in [T, TT] + [lv[k] for lv in applied[:-1] for k in "APR"])
    elif case.coded:
        assert all(applied[l][key].handle.value_bytes() == applied[l][key].nnz for l, key in case.coded)

    # the case contains what it is named for, by the row blocks the kernels will walk
    for line in cases.check_structure(case, K, lambda where: _matrix_at(applied, where).handle.row_blocks()):
        print(line)

    # 1. the joint cycle, 2. the component-by-component cycle of the single-vector kernels
    _check_aux(eng, aux, name, K, storage, n_out, "joint")
    with eng.overrides(amg_batch=0):
        _check_aux(eng, aux, name, K, storage, n_out, "sequential")

    # 3. the plain handle: against long double, and the re-plan has not moved a bit of it
    for s, was in zip(SCALES, before):
        want, bound, tol = cases.cycle_reference(name, storage, s, 12)
        ref.check(was, want, bound, tol, "%s %s plain handle bscale=%g" % (name, storage, s))
        np.testing.assert_array_equal(cases.apply(eng, plain, s, b0, case.n0), was)

    # 4. nothing of one application is left for the next
    b1, b2 = cases.right_hand_side(n_out, 11), cases.right_hand_side(n_out, 13)
    first = cases.apply(eng, aux, 1.0, b1, n_out)
    want, bound, tol = cases.auxiliary_reference(name, K, storage, 1.0, 13)
    ref.check(cases.apply(eng, aux, 1.0, b2, n_out), want, bound, tol, "%s K=%d %s second right-hand side" % (name, K, storage))
    np.testing.assert_array_equal(cases.apply(eng, aux, 1.0, b1, n_out), first)


@pytest.mark.parametrize("storage", ["fp64", "fp32"])
def test_two_components_reach_the_tail_loop_on_a_million_rows(hip_engine, storage):
    """With K = 2 a row block has more (row, component) pairs than prefetch slots only when the launch plan gives it more
    than 256 rows, which it does from 2 * 256 * 2048 rows on: one hierarchy of that size, one right-hand side."""
    eng = hip_engine
    name, K, bscale = cases.LARGE, 2, -1.5
    case = cases.hierarchy(name)
    applied, _ = cases.engine_levels(case, eng, storage)
    plain = eng.amg_create(applied, case.omega)
    T, TT = cases.engine_transform(name, K, eng, storage)
    aux = eng.amg_create_auxiliary(T.handle, TT.handle, [plain] * K)
    for line in cases.check_structure(case, K, lambda where: _matrix_at(applied, where).handle.row_blocks()):
        print(line)
    want, bound, tol = cases.auxiliary_reference(name, K, storage, bscale, 11)
    b = cases.right_hand_side(T.height, 11)
    joint = cases.apply(eng, aux, bscale, b, T.height)
    print("joint: %.3g" % ref.check(joint, want, bound, tol, "%s %s joint" % (name, storage)))
    with eng.overrides(amg_batch=0):
        print("sequential: %.3g" % ref.check(cases.apply(eng, aux, bscale, b, T.height), want, bound, tol,
                                             "%s %s sequential" % (name, storage)))
    np.testing.assert_array_equal(cases.apply(eng, aux, bscale, b, T.height), joint)


def test_coded_level_leaves_the_cycle_unchanged(hip_engine):
    """value codes on level matrices (nss_csr_code_values): the same doubles, the same products in the same order"""
    eng = hip_engine
    case = cases.hierarchy("coded_level")
    out = {}
    for code in (False, True):
        applied, _ = cases.engine_levels(case, eng, "fp64", code=code)
        plain = eng.amg_create(applied, case.omega)
        T, TT = cases.engine_transform(case.name, 3, eng)
        aux = eng.amg_create_auxiliary(T.handle, TT.handle, [plain] * 3)
        assert all((applied[l][key].handle.value_bytes() == applied[l][key].nnz) == code for l, key in case.coded)
        b = cases.right_hand_side(T.height, 11)
        joint = cases.apply(eng, aux, 1.0, b, T.height)
        with eng.overrides(amg_batch=0):
            out[code] = (joint, cases.apply(eng, aux, 1.0, b, T.height))
    for a, b in zip(out[False], out[True]):
        np.testing.assert_array_equal(a, b)


@pytest.mark.parametrize("storage", ["fp64", "fp32"])
@pytest.mark.parametrize("name", cases.NAMES)
def test_fallbacks_take_the_sequential_cycle(hip_engine, name, storage):
    """one component, four components, and two distinct handles of equal levels: no joint cycle -- the hierarchy keeps its
    launch plans -- and the same bound"""
    eng = hip_engine
    case = cases.hierarchy(name)
    applied, _ = cases.engine_levels(case, eng, storage)
    handles = [eng.amg_create(applied, case.omega) for _ in range(3)]
    gen0 = _generations(applied)
    for K, comps in ((1, handles[:1]), (4, handles[:1] * 4), (2, handles[:2]), (3, handles)):
        T, TT = cases.engine_transform(name, K, eng, storage)
        aux = eng.amg_create_auxiliary(T.handle, TT.handle, comps)
        assert _generations(applied) == gen0, "a hierarchy that is not cycled jointly was re-planned"
        _check_aux(eng, aux, name, K, storage, T.height, "fallback of %d handle(s)" % len(set(map(id, comps))))


@pytest.mark.parametrize("storage", ["fp64", "fp32"])
@pytest.mark.parametrize("K", [2, 3])
def test_shared_one_level_hierarchy_is_cycled_sequentially(hip_engine, K, storage):
    eng = hip_engine
    case = cases.hierarchy("one_level")
    applied, _ = cases.engine_levels(case, eng, storage)
    plain = eng.amg_create(applied, case.omega)
    gen0 = _generations(applied)
    T, TT = cases.engine_transform("one_level", K, eng, storage)
    aux = eng.amg_create_auxiliary(T.handle, TT.handle, [plain] * K)
    assert _generations(applied) == gen0
    _check_aux(eng, aux, "one_level", K, storage, T.height, "one level")
    want, bound, tol = cases.cycle_reference("one_level", storage, -1.5, 12)
    ref.check(cases.apply(eng, plain, -1.5, cases.right_hand_side(case.n0, 12), case.n0), want, bound, tol, "one level, plain")
