"""The long-double reference of the AMG cycle (amg_cycle_reference.py) held against the fp64 restatement of the same cycle
(the numpy checker engine, given the same hand-made levels) on every hierarchy of the joint-cycle GPU test, and the
sharpness of the componentwise check |got_i - ref_i| <= tolerance * E_i: six faults a kernel could have, injected one
at a time into the fp64 restatement, each put the result outside the bound.

Largest observed |err_i| / (tolerance * E_i) of the fp64 restatement over all hierarchies, 1 - 4 components, both
storages and both right-hand-side scales: 0.0061 (auxiliary term) and 0.020 (plain cycle; on the one-level hierarchy, a
single dense product) -- far below 1: the inputs are well inside the bound."""
import numpy as np
import pytest
import scipy.sparse as sp

import amg_cycle_cases as cases
import amg_cycle_reference as ref
from oracle.numpy_engine import NumpyEngine

SCALES = (1.0, -1.5)


def _handles(case, K, storage, engine=None):
    engine = engine or NumpyEngine()
    applied, _ = cases.engine_levels(case, engine, storage)
    plain = engine.amg_create(applied, case.omega)
    T, TT = cases.engine_transform(case.name, K, engine, storage)
    return engine, plain, engine.amg_create_auxiliary(T.handle, TT.handle, [plain] * K), T.height


@pytest.mark.parametrize("storage", ["fp64", "fp32"])
@pytest.mark.parametrize("name", cases.NAMES + ["one_level"])
def test_fp64_restatement_is_inside_the_bound(name, storage):
    case = cases.hierarchy(name)
    worst = 0.0
    for K in (1, 2, 3, 4):
        engine, plain, aux, n_out = _handles(case, K, storage)
        for bscale in SCALES:
            want, bound, tol = cases.auxiliary_reference(name, K, storage, bscale, 11)
            got = cases.apply(engine, aux, bscale, cases.right_hand_side(n_out, 11), n_out)
            worst = max(worst, ref.check(got, want, bound, tol, "%s K=%d %s" % (name, K, storage)))
    for bscale in SCALES:
        want, bound, tol = cases.cycle_reference(name, storage, bscale, 12)
        got = cases.apply(engine, plain, bscale, cases.right_hand_side(case.n0, 12), case.n0)
        plain_ratio = ref.check(got, want, bound, tol, "%s plain %s" % (name, storage))
        print("%s %s: worst ratio auxiliary %.3g, plain %.3g (tolerance %.3g)" % (name, storage, worst, plain_ratio, tol))
        assert max(worst, plain_ratio) < 0.25            # nowhere near 1: else the inputs are too ill-conditioned


def test_fp64_restatement_is_inside_the_bound_on_a_million_rows():
    name, K, bscale = cases.LARGE, 2, -1.5
    engine, _, aux, n_out = _handles(cases.hierarchy(name), K, "fp64")
    want, bound, tol = cases.auxiliary_reference(name, K, "fp64", bscale, 11)
    got = cases.apply(engine, aux, bscale, cases.right_hand_side(n_out, 11), n_out)
    assert ref.check(got, want, bound, tol, name) < 0.25


def test_the_tolerance_is_the_derived_one():
    """2 * 2^-53 * sum over the kernels of (longest row + 3), spelled out for one hierarchy"""
    case = cases.hierarchy("full_blocks")
    T = cases.transform("full_blocks", 2)
    rows = lambda m: int(np.diff(m.indptr).max())
    total = rows(T) + 3 + rows(T.T.tocsr()) + 3 + rows(case.inv) + 3
    for lv in case.levels:
        total += 4 + 2 * (rows(lv["A"]) + 3) + rows(lv["R"]) + 3 + rows(lv["P"]) + 3
    assert rows(case.levels[0]["A"]) == 3001
    assert ref.tolerance(case.levels, case.inv, T) == 2.0 * 2.0 ** -53 * total
    assert 2e-12 < ref.tolerance(case.levels, case.inv, T) < 4e-12


def test_long_double_is_wider_than_fp64():
    assert np.finfo(np.longdouble).eps < 1e-18


# ---- sharpness: faults injected into the fp64 restatement ---------------------------------------------------------------
def _with(case, where, mat):
    """a copy of `case` with the matrix at `where` replaced"""
    levels = [dict(lv) for lv in case.levels]
    coarse = dict(case.coarse)
    if where == "inv":
        coarse["inv"] = mat
    else:
        levels[where[0]][where[1]] = mat
    return cases.Hierarchy(case.name, levels, coarse)


def _drop(mat, position):
    out = sp.csr_matrix(mat, copy=True)
    out.data[position] = 0.0
    return out


def _row_takes_the_next_rows_bounds(mat, i):
    mat = mat.tocsr()
    rows = [mat[r] for r in range(mat.shape[0])]
    rows[i] = rows[i + 1]
    return sp.vstack(rows).tocsr()


class _FaultyEngine(NumpyEngine):
    """the checker engine's cycle with one of the faults that are no change of a matrix"""

    def __init__(self, fault):
        self.fault = fault

    def amg_apply(self, h, bscale, b, x):
        if "T" not in h or self.fault[0] != "component":
            return super().amg_apply(h, bscale, b, x)
        _, i, k = self.fault
        K = len(h["comps"])
        n = h["comps"][0]["levels"][0]["n"]
        r = (h["TT"] @ (bscale * b)).reshape(K, n)
        z = np.stack([self._vcycle(h["comps"][c], 0, r[c]) for c in range(K)])
        z[(k + 1) % K, i] = z[k, i]                        # component k of row i lands in component (k + 1) % K
        x[:] = h["T"] @ z.ravel()

    def _vcycle(self, h, l, b):
        lv, w = h["levels"][l], h["omega"]
        if "inv" in lv:
            return lv["inv"].handle.mat @ b
        A, dinv = lv["A"].handle.mat, lv["dinv"]
        x = w * (dinv * b)
        r = b - A @ x
        bc = lv["R"].handle.mat @ r
        if self.fault[0] == "stale" and self.fault[1] == l:
            bc[self.fault[2]] = self.fault[3]              # the empty row's output is not written
        x = x + lv["P"].handle.mat @ self._vcycle(h, l + 1, bc)
        post = dinv.copy()
        if self.fault[0] == "post" and self.fault[1] == l:
            post[-1] = 1.0                                 # the last row's post-smoothing misses its dinv
        return x + w * (post * (b - A @ x))


def _faults():
    full, coarse, empty = (cases.hierarchy(n) for n in ("full_blocks", "coarse_dense", "empty_rows"))
    out = []
    for key in "APR":                                      # rows 3 (1025 entries) and 4 (3001): blocks of their own
        m = full.levels[0][key]
        out.append(("last entry of the 3001-entry row of %s dropped" % key, _with(full, (0, key), _drop(m, m.indptr[5] - 1)), None))
        out.append(("last entry of the 1025-entry row of %s dropped" % key, _with(full, (0, key), _drop(m, m.indptr[4] - 1)), None))
        # rows 1 and 2 (1023 + 1 entries) share a row block of exactly 1024 products, row 0 has one to itself
        out.append(("entry 1024 of the 1023 + 1 block of %s dropped" % key, _with(full, (0, key), _drop(m, m.indptr[3] - 1)), None))
        out.append(("entry 1024 of the full row of %s dropped" % key, _with(full, (0, key), _drop(m, m.indptr[1] - 1)), None))
        out.append(("row 2 of %s read with the bounds of row 3 (block boundary)" % key,
                    _with(full, (0, key), _row_takes_the_next_rows_bounds(m, 2)), None))
        out.append(("row 0 of %s read with the bounds of row 1 (block boundary)" % key,
                    _with(full, (0, key), _row_takes_the_next_rows_bounds(m, 0)), None))
    inv = coarse.inv
    row = int(coarse.levels[0]["P"].indices[5])            # (a coarse row that P reads: the others do not reach the result)
    out.append(("last entry of a row of the dense coarse inverse dropped", _with(coarse, "inv", _drop(inv, inv.indptr[row + 1] - 1)), None))
    deep, rag = cases.hierarchy("thresholds"), cases.hierarchy("ragged")
    m = deep.levels[3]["A"]                                # the deepest level operator (L = 2, four levels down)
    out.append(("last entry of a row of the level-3 operator dropped", _with(deep, (3, "A"), _drop(m, m.indptr[101] - 1)), None))
    m = rag.levels[0]["A"]                                 # a short row of the 64-row block [30, 94) behind the long rows
    out.append(("last entry of a short row of the ragged operator dropped", _with(rag, (0, "A"), _drop(m, m.indptr[61] - 1)), None))
    for l, row in ((0, 0), (0, 599), (0, 300), (1, 25)):
        assert empty.levels[l]["R"].indptr[row] == empty.levels[l]["R"].indptr[row + 1]
        out.append(("empty row %d of R on level %d keeps a stale value" % (row, l), empty, ("stale", l, row, 1e-6)))
    for name in ("short_rows", "full_blocks", "empty_rows"):
        case = cases.hierarchy(name)
        # (a fault shows only where something reads the entry it spoils: T has columns without entries, P too)
        read = [np.diff(cases.transform(name, K).tocsc().indptr).reshape(K, case.n0) > 0 for K in (2, 3)]
        mid = next(i for i in range(case.n0 // 2, case.n0) if all(r[1, i] for r in read))
        last = next(i for i in range(case.n0 - 1, 0, -1) if all(r[0, i] for r in read))
        out.append(("component 0 of a row written into component 1 (%s)" % name, case, ("component", mid, 0)))
        out.append(("last component of a row written into component 0 (%s)" % name, case, ("component", last, -1)))
        for l in range(len(case.levels)):
            # (... and the last row of a coarser level has a residual only if its row of R is not empty)
            if l == 0 or (np.diff(case.levels[l - 1]["P"].tocsc().indptr)[-1] > 0
                          and np.diff(case.levels[l - 1]["R"].indptr)[-1] > 0):
                out.append(("post-smoothing without dinv on the last row of level %d (%s)" % (l, name), case, ("post", l)))
    return out


FAULTS = _faults()


@pytest.mark.parametrize("what", [f[0] for f in FAULTS])
def test_an_injected_fault_is_outside_the_bound(what):
    _, case, fault = FAULTS[[f[0] for f in FAULTS].index(what)]
    name = case.name
    for K in (2, 3):
        if fault is not None and fault[0] == "component" and fault[2] < 0:
            fault = ("component", fault[1], K - 1)
        engine, _, aux, n_out = _handles(case, K, "fp64", _FaultyEngine(fault) if fault else None)
        want, bound, tol = cases.auxiliary_reference(name, K, "fp64", 1.0, 11)
        got = cases.apply(engine, aux, 1.0, cases.right_hand_side(n_out, 11), n_out)
        ratio = ref.worst_ratio(got, want, bound, tol)
        print("%s, K = %d: |err_i| / (tolerance * E_i) reaches %.3g" % (what, K, ratio))
        assert ratio > 1.0, (what, K, ratio)
        # ... and without the fault the same engine path is inside it
        clean = _handles(cases.hierarchy(name), K, "fp64", _FaultyEngine(("none",)))
        assert ref.worst_ratio(cases.apply(clean[0], clean[2], 1.0, cases.right_hand_side(n_out, 11), n_out),
                               want, bound, tol) < 0.25
