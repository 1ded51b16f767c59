"""The references and cases of the set-up tests (setup_reference.py, setup_cases.py) checked on their own, without a GPU:
every case contains the situation it is named for, the two references of the integer sparse products agree, the fp64
restatement of the block inversion stays inside GAMMA * 2^-53 * E of the long-double solve (and the measured factor behind
GAMMA is the one written down), and that bound tells the five injected faults from a correct kernel."""

import numpy as np
import pytest
import scipy.sparse as sp

import amg_cycle_reference as cyc
import setup_cases as cases
import setup_reference as sr


def _assert_situation(name, situation, figures=None):
    print(name, figures if figures is not None else "")
    missing = [what for what, holds in situation.items() if not holds]
    assert not missing, "%s does not contain: %s" % (name, "; ".join(missing))


def _restatement(case, inverse=None, stored=None, idx=None):
    """largest |err_i| / (2^-53 E_i) of an fp64 application against the long-double solve, over the case's two vectors"""
    if stored is None:
        inv = sr.block_jacobi_fp64(case.A, case.idx)[0] if inverse is None else inverse
        stored = sr.stored_inverse(inv)[1]
    worst = 0.0
    for x in cases.bjac_vectors(case)[0]:
        got = sr.apply_blocks(stored, case.idx if idx is None else idx, x)
        worst = max(worst, sr.ratio(got, sr.block_solve_ld(case.A, case.idx, x), sr.block_bound(case.A, case.idx, x)))
    return worst


# ---- block Jacobi --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(cases.BJAC_BUILDERS) + list(cases.BJAC_SINGULAR))
def test_block_case_contains_its_situation(name):
    case = cases.bjac_case(name)
    _assert_situation(name, case.situation, case.figures)
    assert case.idx.dtype == np.int32 and case.A.shape == (case.n, case.n)
    flat = case.idx[case.idx >= 0]
    assert np.unique(flat).size == flat.size and flat.max() < case.n


def test_long_double_solve_solves():
    """the reference itself: A_bb y_b = x_b to long-double accuracy, padding and uncovered dofs 0"""
    for name in ("saddle[5]", "interior_padding", "permutation_like"):
        case = cases.bjac_case(name)
        x = cases.bjac_vectors(case)[0][0]
        y = sr.block_solve_ld(case.A, case.idx, x)
        M = sr.gather_blocks(case.A, case.idx, sr.LD)
        yb = np.where(case.idx.T >= 0, y[np.maximum(case.idx.T, 0)], 0)
        xb = np.where(case.idx.T >= 0, x[np.maximum(case.idx.T, 0)], 0).astype(sr.LD)
        res = np.abs(np.einsum("brc,bc->br", M, yb) - xb)
        scale = np.einsum("brc,bc->br", np.abs(M), np.abs(yb)) + np.abs(xb)
        assert np.all(res <= 64 * np.finfo(sr.LD).eps * scale)
        assert np.all(y[~sr.covered(case.idx, case.n)] == 0)


def test_restatement_stays_inside_gamma_and_gamma_is_four_times_the_measured_ratio():
    worst, where = 0.0, None
    for name in cases.BJAC_BUILDERS:
        r = _restatement(cases.bjac_case(name))
        print("%-24s |err_i| / (2^-53 E_i) <= %.3g" % (name, r))
        assert r <= sr.GAMMA, name
        if r > worst:
            worst, where = r, name
    print("largest ratio of the fp64 restatement: %.4g (%s); GAMMA = %.4g" % (worst, where, sr.GAMMA))
    assert sr.GAMMA == 4.0 * sr.MEASURED_RATIO
    assert 0.9 * sr.MEASURED_RATIO <= worst <= sr.MEASURED_RATIO, "setup_reference.MEASURED_RATIO is not the measured ratio"


def _transposed(case):
    return dict(stored=np.swapaxes(sr.block_jacobi_fp64(case.A, case.idx)[0], 1, 2).copy())


def _padding_dropped(case):
    """the block inverted without its padding slots (the dofs moved up), applied through the table as it is"""
    idx = case.idx
    compact = -np.ones_like(idx)
    for b in range(idx.shape[1]):
        d = idx[idx[:, b] >= 0, b]
        compact[:d.size, b] = d
    return dict(stored=sr.stored_inverse(sr.block_jacobi_fp64(case.A, compact)[0])[1])


FAULTS = [
    ("no pivoting", lambda c: dict(inverse=sr.block_jacobi_fp64(c.A, c.idx, pivoting=False)[0]), "swap_2x2[257]"),
    ("the swap applied to the left half only", lambda c: dict(inverse=sr.block_jacobi_fp64(c.A, c.idx, swap_left_only=True)[0]), "saddle[5]"),
    ("the transposed inverse of a non-symmetric block", _transposed, "repeated_pivoted"),
    ("the packed average although one block is asymmetric",
     lambda c: dict(stored=sr.stored_inverse(sr.block_jacobi_fp64(c.A, c.idx)[0], force_packed=True)[1]), "one_asymmetric_block"),
    ("padding rows dropped instead of identity", _padding_dropped, "interior_padding"),
]


@pytest.mark.parametrize("what,inject,named", FAULTS, ids=[f[0] for f in FAULTS])
def test_injected_fault_lands_outside_the_bound(what, inject, named):
    outside = {}
    for name in cases.BJAC_BUILDERS:
        case = cases.bjac_case(name)
        r = _restatement(case, **inject(case))
        if r > sr.GAMMA:
            outside[name] = r
    print("%s: outside GAMMA * 2^-53 * E on %s" % (what, ", ".join("%s (%.3g)" % kv for kv in outside.items())))
    assert named in outside, "%s is inside the bound on %s" % (what, named)
    assert outside[named] > 100 * sr.GAMMA


def test_symmetric_decision_of_the_twins():
    one, tiny = cases.bjac_case("one_asymmetric_block"), cases.bjac_case("tiny_asymmetry")
    assert not one.packed and tiny.packed
    inv = sr.block_jacobi_fp64(tiny.A, tiny.idx)[0]
    packed, stored = sr.stored_inverse(inv)
    assert packed and np.array_equal(stored, np.swapaxes(stored, 1, 2)) and not np.array_equal(inv, np.swapaxes(inv, 1, 2))


# ---- sparse products -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(cases.SPGEMM_BUILDERS))
def test_spgemm_case_and_its_two_references(name):
    from oracle import krylov_ref as kr
    case = cases.spgemm_case(name)
    _assert_situation(name, case.situation, case.figures)
    C = kr.sa_spgemm(case.X, case.Y)
    assert C.has_sorted_indices and np.all(C.data != 0)
    if case.integer:                                       # small integers: the dense product is exact
        D = sp.csr_matrix(case.X.toarray() @ case.Y.toarray())
        D.sort_indices()
        np.testing.assert_array_equal(C.indptr, D.indptr)
        np.testing.assert_array_equal(C.indices, D.indices)
        np.testing.assert_array_equal(C.data, D.data)


@pytest.mark.parametrize("m,n", cases.TRANSPOSE_SHAPES)
def test_transpose_case_and_reference(m, n):
    M, situation = cases.transpose_case(m, n)
    _assert_situation("transpose %dx%d" % (m, n), situation, dict(nnz=M.nnz))
    trow, tcol, tval, shape = sr.transpose_stable(M.indptr, M.indices, M.data, M.shape)
    T = M.T.tocsr()
    T.sort_indices()
    assert shape == T.shape
    np.testing.assert_array_equal(trow, T.indptr)
    np.testing.assert_array_equal(tcol, T.indices)
    np.testing.assert_array_equal(tval, T.data)
    assert all(np.all(np.diff(tcol[a:b]) > 0) for a, b in zip(trow[:-1], trow[1:]))


# ---- aggregation and prolongator -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(cases.AGG_BUILDERS))
def test_aggregation_case_contains_its_situation(name):
    case = cases.agg_case(name)
    _assert_situation(name, case.situation, case.figures)


@pytest.mark.parametrize("name", list(cases.PRO_BUILDERS))
def test_prolongator_case_contains_its_situation(name):
    _assert_situation(name, cases.PRO_BUILDERS[name]().situation)


# ---- permutation and launch plan -------------------------------------------------------------------------------------------
def test_permute_reference_and_cases():
    sources = cases.permute_sources()
    lens = np.diff(sources["ragged"].indptr)
    assert sorted(set(lens.tolist())) == [0, 1, 7, 40] and sources["ragged"].shape == (300, 300)
    unsorted = 0
    for case in cases.all_permute_cases():
        rowptr, col, val, shape = sr.permute_rows_cols(case.source, case.rows, case.colmap, case.ncols_out)
        got = sr.as_stored(rowptr, col, val, shape)
        want = sp.csr_matrix((case.source.data, case.colmap[case.source.indices], case.source.indptr),
                             shape=(case.source.shape[0], case.ncols_out))[case.rows] if case.rows.size else sp.csr_matrix(shape)
        assert (got != want).nnz == 0 and got.nnz == want.nnz, case.name
        unsorted += any(np.any(np.diff(col[a:b]) < 0) for a, b in zip(rowptr[:-1], rowptr[1:]))
        if case.row_pos is not None:                        # what the case asks of the plan is satisfiable
            assert case.row_pos.dtype == np.uint8 and case.row_pos.size == case.rows.size and case.row_pos[0] == 0
            sizes = np.diff(np.append(np.flatnonzero(case.row_pos == 0), case.rows.size))
            assert sizes.max() > case.max_rows or case.max_rows >= 12
            assert set(range(1, 13)) <= set(sizes.tolist()) | {int(sizes[-1])}
            assert all(c == case.rows.size or case.row_pos[c] == 0 for c in ([] if case.cuts is None else case.cuts))
        x = np.random.default_rng(5).standard_normal(case.ncols_out)
        np.testing.assert_allclose(np.asarray(cyc.spmv_ld(got, x), dtype=float), want @ x, rtol=0, atol=1e-12 * (abs(want) @ abs(x)).max() if want.nnz else 0)
    assert unsorted >= 10, "the column maps leave the rows sorted"


def test_plan_respects_rejects_bad_plans():
    pos = np.array([0, 1, 2, 0, 0, 1, 0, 1, 2, 3, 4, 5], dtype=np.uint8)      # groups of 3, 1, 2, 6 rows
    good = [0, 3, 6, 12]
    assert sr.plan_respects(good, [0, 6, 6, 12], 3, pos) is None             # the group of 6 alone may exceed max_rows
    assert sr.plan_respects([0, 12], None, 0, pos) is None
    assert "crosses the cut" in sr.plan_respects([0, 3, 12], [6], 0, pos)
    assert "splits a group" in sr.plan_respects([0, 2, 6, 12], None, 0, pos)
    assert "splits a group" in sr.plan_respects([0, 3, 6, 9, 12], None, 3, pos)
    assert "more than 3" in sr.plan_respects([0, 4, 6, 12], None, 3, pos)    # two groups, four rows
    assert "more than 2" in sr.plan_respects([0, 3, 6, 12], None, 2, None)
    assert "ascending" in sr.plan_respects([0, 3, 3, 12], None, 0, None)
    assert "entries" in sr.plan_respects([0, 3, 11], None, 0, pos)


def test_luby_rounds_counts_the_rounds_of_the_restatement():
    from oracle import krylov_ref as kr
    case = cases.agg_case("luby_worst_case")
    g = kr.sa_strength_graph(case.A, case.theta)
    assert sr.luby_rounds(g, case.priority) == 86 and kr.sa_mis2(g, case.priority).sum() == 86
