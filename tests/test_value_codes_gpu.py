"""One-byte value codes (nss_csr_code_values): a matrix with at most 256 distinct 64-bit value patterns streams one
byte per entry, the index into a dictionary the kernels hold in LDS, instead of the 8-byte value.  The products are the
same doubles times the same operands and the sums keep their order, so every result must be IDENTICAL -- compared on
the uint64 views throughout -- to what the uncoded matrix gives."""

import contextlib
import io
import re

import numpy as np
import pytest
import scipy.sparse as sp

from staggered_grid import mac_stokes

pytestmark = pytest.mark.gpu

DICT_BYTES = 8 * 256


class Form:
    def __init__(self, mat):
        self.mat, self.condense = mat, False


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def upload(eng, csr):
    csr = sp.csr_matrix(csr)
    csr.sort_indices()
    return eng.csr_create(csr.shape[0], csr.shape[1], csr.indptr, csr.indices, csr.data)


def spmv(eng, h, x, y0, alpha=-1.75, beta=0.625):
    xb, yb = eng.zeros(h.n), eng.zeros(h.m)
    eng.upload(x, xb)
    eng.upload(y0, yb)
    eng.csr_spmv(h, alpha, xb, beta, yb)
    eng.synchronize()
    return eng.to_host(yb).copy()


def operands(csr, seed=0):
    rng = np.random.default_rng(seed)
    return rng.standard_normal(csr.shape[1]), rng.standard_normal(csr.shape[0])


def expected_bytes(info):
    """nss_csr_info's algorithmic_bytes of a coded matrix: the value stream at 1 byte per entry plus the 2-KiB dictionary
    per row block; the fixed-width form rows x (8 + 2)."""
    m, n, nnz, nblk = info["rows"], info["cols"], info["nnz"], info["row_blocks"]
    if info["operand_form"] == "rows":
        return m * (8 + 2) + DICT_BYTES * nblk + 8 * n + 8 * m
    if info["index_bytes"] == 2:
        index = 2 * (nnz // info["index_group"]) + 4 * (32 if info["operand_form"] == "staged" else 16) * nblk
    else:
        index = 4 * nnz
    return index + nnz + DICT_BYTES * nblk + 4 * (m + 1) + 8 * n + 8 * m


# ---- 1. plain SpMV ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim,n", [(3, 12), (2, 40)])
@pytest.mark.parametrize("rows_kernel", [False, True])
def test_plain_spmv_coded_equals_uncoded_twin(hip_engine, dim, n, rows_kernel):
    s = mac_stokes(dim, n)
    for name, mat in (("A", s.A), ("B", s.B), ("BT", s.B.T.tocsr())):
        x, y0 = operands(mat)
        with hip_engine.overrides(direct_rows=0 if rows_kernel else -1):
            plain, coded = upload(hip_engine, mat), upload(hip_engine, mat)
        assert coded.code_values()
        info = coded.info()
        assert info["value_bytes"] == info["nnz"] and plain.info()["value_bytes"] == 8 * info["nnz"]
        if name == "BT":
            assert (info["operand_form"] == "rows") == rows_kernel
        else:
            assert info["operand_form"] == "staged", info              # (the form the headline's A and B take)
        assert same_bits(spmv(hip_engine, coded, x, y0), spmv(hip_engine, plain, x, y0)), name


def test_coded_spmv_over_the_lanes_per_row_regimes_and_column_forms(hip_engine):
    """The coded stream kernel at every lanes-per-row value of the launch plan and in every column form (the loops only
    reach it with the short rows of the Stokes blocks): identical bits to the uncoded twin."""
    import lane_regimes
    seen, forms = set(), set()
    for name, make, lanes, form in lane_regimes.CASES:
        mat = make()
        assert distinct_patterns(mat) < 256 and lane_regimes.plan_lanes(mat.nnz / mat.shape[0]) == lanes, name
        x, y0 = operands(mat)
        plain, coded = upload(hip_engine, mat), upload(hip_engine, mat)
        assert coded.code_values(), name
        info = coded.info()
        assert info["lanes_per_row"] == lanes and info["operand_form"] == form, (name, info)
        assert info["value_bytes"] == info["nnz"] == mat.nnz and plain.info()["value_bytes"] == 8 * mat.nnz, (name, info)
        assert same_bits(spmv(hip_engine, coded, x, y0), spmv(hip_engine, plain, x, y0)), name
        seen.add(info["lanes_per_row"])
        forms.add(info["operand_form"])
    assert forms == {"gather32", "gather16", "staged"}
    assert seen == {1, 2, 4, 8, 16, 32, 64}


# ---- 2. dictionary edges -------------------------------------------------------------------------------------------
def random_csr(rng, values, rows=3001, cols=3500, long_row=None):
    """short rows (some empty) whose values are drawn from `values`, every one of them at least once"""
    lengths = rng.integers(0, 8, size=rows)
    lengths[rng.integers(0, rows, size=rows // 10)] = 0
    if long_row is not None:
        lengths[long_row] = 3000
    indptr = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int32)
    nnz = int(indptr[-1])
    if nnz % 256 == 0:
        raise AssertionError("entry count must not be a multiple of 256: change the seed")
    indices = np.concatenate([np.sort(rng.choice(cols, size=k, replace=False)) for k in lengths]).astype(np.int32)
    values = np.asarray(values, dtype=np.float64)
    assert nnz >= len(values)
    data = values[rng.integers(0, len(values), size=nnz)]
    data[rng.permutation(nnz)[:len(values)]] = values
    return sp.csr_matrix((data, indices, indptr), shape=(rows, cols))


def distinct_patterns(csr):
    return len(np.unique(np.ascontiguousarray(csr.data).view(np.uint64)))


@pytest.mark.parametrize("case", ["256", "257", "signed_zeros", "long_row"])
def test_dictionary_edges(hip_engine, case):
    rng = np.random.default_rng(7)
    long_row = None
    if case in ("256", "257"):
        values = rng.standard_normal(int(case))
    elif case == "signed_zeros":
        values = np.array([0.0, -0.0, 1.5, -1.5, 3.0e-310])            # (a subnormal beside the two zeros)
    else:
        values, long_row = np.array([2.0, -1.0, 0.25, 1.0 / 3.0]), 1234
    mat = random_csr(rng, values, long_row=long_row)
    assert distinct_patterns(mat) == len(values)
    x, y0 = operands(mat, 1)                                             # finite: no +-inf meets a zero
    plain, coded = upload(hip_engine, mat), upload(hip_engine, mat)
    nnz = mat.nnz
    want = spmv(hip_engine, plain, x, y0)
    if case == "257":
        assert not coded.code_values()
        assert coded.info()["value_bytes"] == 8 * nnz
    else:
        assert coded.code_values()
        assert coded.info()["value_bytes"] == nnz
    assert same_bits(spmv(hip_engine, coded, x, y0), want)
    assert same_bits(hip_engine.csr_to_host(coded)[2], mat.data)
    if case == "signed_zeros":
        # the sign of a zero product is visible in a row whose only entry is -0.0 times a positive operand
        one = sp.csr_matrix((np.array([-0.0, 0.0, 1.0]), np.array([0, 0, 0]), np.array([0, 1, 2, 3])), shape=(3, 1))
        h = upload(hip_engine, one)
        assert h.code_values()
        y = spmv(hip_engine, h, np.array([2.0]), np.zeros(3), alpha=1.0, beta=0.0)
        assert same_bits(y, spmv(hip_engine, upload(hip_engine, one), np.array([2.0]), np.zeros(3), alpha=1.0, beta=0.0))


# ---- 3. set-up paths -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("how", ["round", "narrow"])
def test_writers_of_the_values_drop_the_codes(hip_engine, how):
    s = mac_stokes(2, 40)
    # values that are not fp32 numbers, so that the rounding changes them
    mat = sp.csr_matrix(s.A * (1.0 / 3.0))
    x, y0 = operands(mat)
    plain, coded = upload(hip_engine, mat), upload(hip_engine, mat)
    assert coded.code_values() and coded.info()["value_bytes"] == mat.nnz
    for h in (plain, coded):
        (hip_engine.csr_round_f32 if how == "round" else hip_engine.csr_narrow_f32)(h)
    assert coded.info()["value_bytes"] == (8 if how == "round" else 4) * mat.nnz
    got = spmv(hip_engine, coded, x, y0)
    assert same_bits(got, spmv(hip_engine, plain, x, y0))
    assert not same_bits(got, spmv(hip_engine, upload(hip_engine, mat), x, y0))      # (the rounding did happen)
    assert same_bits(hip_engine.csr_to_host(coded)[2], mat.data.astype(np.float32).astype(np.float64))


@pytest.mark.parametrize("rows_kernel", [False, True])
def test_replans_keep_the_codes(hip_engine, rows_kernel):
    import hipla
    with hip_engine.overrides(direct_rows=0 if rows_kernel else -1, fuse_bjac=1):
        s = mac_stokes(2, 40)
        A = hipla.SparseMatrix.from_scipy(s.A)
        B, BT = hipla.SparseMatrix.from_scipy(s.B), hipla.SparseMatrix.from_scipy(s.B.T.tocsr())
        pre = hipla.BlockJacobi(A, s.line_blocks(2))
        for mat, host, blocks in ((B, s.B, False), (BT, s.B.T.tocsr(), True)):
            x, y0 = operands(host)
            want = spmv(hip_engine, upload(hip_engine, host), x, y0)
            h = mat.handle
            assert h.code_values()
            assert same_bits(spmv(hip_engine, h, x, y0), want)
            gen = h.plan_generation()
            if blocks:
                assert h.plan_for_blocks(pre.handle)
                assert h.plan_generation() != gen          # (it really was re-planned, the fixed-width copy rebuilt)
            else:
                h.plan_for_pairs()
            info = h.info()
            assert info["value_bytes"] == info["nnz"] and info["algorithmic_bytes"] == expected_bytes(info)
            assert same_bits(spmv(hip_engine, h, x, y0), want)
            assert same_bits(hip_engine.csr_to_host(h)[2], sp.csr_matrix(host).data)


# ---- 4. reporting --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows_kernel", [False, True])
def test_reported_bytes_of_a_coded_matrix(hip_engine, rows_kernel):
    s = mac_stokes(3, 12)
    forms = set()
    for mat in (s.A, s.B, s.B.T.tocsr(), random_csr(np.random.default_rng(3), [1.0, 2.0, 4.0])):
        with hip_engine.overrides(direct_rows=0 if rows_kernel else -1):
            h = upload(hip_engine, mat)
        before = h.info()
        assert before["value_bytes"] == 8 * before["nnz"]
        assert h.code_values()
        info = h.info()
        forms.add(info["operand_form"])
        assert info["value_bytes"] == info["nnz"]
        assert info["algorithmic_bytes"] == expected_bytes(info)
        assert info["algorithmic_bytes"] < before["algorithmic_bytes"]
        with hip_engine.overrides(value_codes=0):                       # never: the kernels read the 8-byte values again
            assert h.info() == before
    assert ("rows" in forms) == rows_kernel


# ---- 5. / 6. the loop ------------------------------------------------------------------------------------------------
def run_bpcg(s, pre, nit=30):
    """(error history, u, p, what the three matrices report) of `nit` iterations with the overrides in force"""
    import hipla
    from solvers.bramblepasciak_new import BramblePasciakCG
    A, B = hipla.SparseMatrix.from_scipy(s.A), hipla.SparseMatrix.from_scipy(s.B)
    preA = hipla.JacobiPreconditioner(A) if pre == "point" else hipla.BlockJacobi(A, s.line_blocks(3))
    f, g = s.rhs(0)
    sol = hipla.BlockVector([hipla.Vector(s.n_u), hipla.Vector(s.n_p)])
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        BramblePasciakCG(Form(A), Form(B), None, hipla.Vector.from_numpy(f), hipla.Vector.from_numpy(g), preA,
                         hipla.DiagonalMatrix(1.0 / s.mass), sol, tol=0.0, maxsteps=nit, printrates=True)
    hist = np.array([float(m) for m in re.findall(r"it =\s+\d+\s+err =\s+(\S+)", out.getvalue())])
    infos = [m.handle.info() for m in (A, B, B.CreateTranspose())]
    x = sol.numpy()
    return hist, x[:s.n_u].copy(), x[s.n_u:].copy(), infos


@pytest.mark.parametrize("dim,n", [(3, 12), (2, 40)])
@pytest.mark.parametrize("pre,fuse", [("block", 0), ("point", 0), ("block", 1)])
@pytest.mark.parametrize("rows_kernel", [False, True])
def test_loop_with_codes_equals_loop_without(hip_engine, dim, n, pre, fuse, rows_kernel):
    """rows_kernel: B^T takes the row-per-lane kernel and C1 its streaming-load variant, as at the headline size"""
    plans = dict(fuse_bjac=fuse, direct_rows=0, stream_loads=1) if rows_kernel else dict(fuse_bjac=fuse)
    s = mac_stokes(dim, n)
    with hip_engine.overrides(value_codes=1, **plans):
        coded = run_bpcg(s, pre)
    for info in coded[3]:                                                # the coded run really was coded
        assert info["value_bytes"] == info["nnz"], info
    assert (coded[3][2]["operand_form"] == "rows") == rows_kernel
    with hip_engine.overrides(value_codes=0, **plans):
        plain = run_bpcg(s, pre)
    for info in plain[3]:
        assert info["value_bytes"] == 8 * info["nnz"], info
    assert len(coded[0]) >= 30 and np.all(np.isfinite(coded[0])) and coded[0][-1] < coded[0][0]
    for a, b in zip(coded[:3], plain[:3]):
        assert same_bits(a, b)


def test_all_or_nothing(hip_engine):
    s = mac_stokes(3, 8).inflate(12)
    assert distinct_patterns(sp.csr_matrix(s.A)) > 256
    with hip_engine.overrides(value_codes=1):
        forced = run_bpcg(s, "point")
    for info in forced[3]:                                               # A does not qualify: nobody is coded
        assert info["value_bytes"] == 8 * info["nnz"], info
    with hip_engine.overrides(value_codes=0):
        plain = run_bpcg(s, "point")
    for a, b in zip(forced[:3], plain[:3]):
        assert same_bits(a, b)
    # B has few patterns but one column index per group of entries: the grouped kernels have no coded form, so it is
    # refused too and keeps reporting 8 bytes per entry
    assert distinct_patterns(sp.csr_matrix(s.B)) <= 256
    h = upload(hip_engine, s.B)
    if h.info()["index_group"] > 1:
        assert not h.code_values() and h.info()["value_bytes"] == 8 * h.nnz
