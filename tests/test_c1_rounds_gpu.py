"""The row-per-lane kernel (csr_direct_kernel) issues a row block's loads in three rounds: full and partial row blocks
take separate straight-line bodies, partial blocks load from a clamped row, padding slots gather from column 0 and are
discarded by a select, C1's epilogue operands are requested up front, and ctrl / scal come through scalar loads.  None
of that may change a bit: every result is compared -- on the uint64 views -- with the stream kernel's on the same matrix
(same products, same order of the row sum)."""

import contextlib
import io

import numpy as np
import pytest
import scipy.sparse as sp

from staggered_grid import mac_stokes

pytestmark = pytest.mark.gpu


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


def spmv(eng, h, x, y0, alpha, beta):
    xb, yb = eng.zeros(h.n), eng.zeros(h.m)
    eng.upload(x, xb)
    eng.upload(y0, yb)
    eng.csr_spmv(h, alpha, xb, beta, yb)
    eng.synchronize()
    return eng.to_host(yb).copy()


FULL_BLOCK_ROWS = 2048 * 512      # from here on the launch plan gives such a matrix row blocks of 512 rows (two per lane)


def short_rows(rows, seed):
    """rows of 0, 1 and 2 entries (every length present from 3 rows on), values from a handful of patterns -- among
    them -0.0 and a negative value, so that the sign of a zero row sum is visible"""
    rng = np.random.default_rng(seed)
    cols = max(3, rows // 2 + 7)
    lengths = rng.integers(0, 3, size=rows)
    lengths[:3] = [0, 1, 2] if rows >= 3 else 2
    first = rng.integers(0, cols - 1, size=rows)
    second = first + 1 + np.floor(rng.random(rows) * (cols - 1 - first)).astype(np.int64)      # in (first, cols)
    slots = np.stack([first, second], axis=1)
    keep = np.arange(2)[None, :] < lengths[:, None]
    indices = slots[keep].astype(np.int32)
    indptr = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int32)
    values = np.array([1.5, -2.25, 1.0 / 3.0, -0.0, 0.0, 7.0e-3])
    data = values[rng.integers(0, len(values), size=int(indptr[-1]))]
    return sp.csr_matrix((data, indices, indptr), shape=(rows, cols))


def spmv_matrices():
    """(name, matrix, row blocks of the row-per-lane plan).  Below FULL_BLOCK_ROWS rows the plan fills the chip with
    256-row blocks: the second row of every lane is past the end (clamped loads); the last entry has 2048 full
    512-row blocks -- the body without a per-lane predicate -- and a partial one."""
    out = [("random_%d" % rows, short_rows(rows, rows), -(-rows // 256)) for rows in (1, 511, 512, 513, 1300)]
    out.append(("BT_3d_12", mac_stokes(3, 12).B.T.tocsr(), None))
    out.append(("BT_2d_40", mac_stokes(2, 40).B.T.tocsr(), None))
    out.append(("random_full_blocks", short_rows(FULL_BLOCK_ROWS + 300, 5), 2049))
    return out


# ---- 1. plain SpMV: row-per-lane kernel against the stream kernel ----------------------------------------------------
@pytest.mark.parametrize("coded", [False, True])
def test_rows_kernel_spmv_equals_stream_kernel(hip_engine, coded):
    for name, mat, blocks in spmv_matrices():
        rng = np.random.default_rng(11)
        x, y0 = rng.standard_normal(mat.shape[1]), rng.standard_normal(mat.shape[0])
        with hip_engine.overrides(direct_rows=-1):
            stream = upload(hip_engine, mat)
        with hip_engine.overrides(direct_rows=0):
            rows = upload(hip_engine, mat)
        if coded:
            assert stream.code_values() and rows.code_values(), name
        assert rows.info()["operand_form"] == "rows" and stream.info()["operand_form"] != "rows", name
        assert blocks is None or rows.info()["row_blocks"] == blocks, (name, rows.info())
        for alpha, beta in ((-1.75, 0.625), (1.0, 0.0)):
            got, want = spmv(hip_engine, rows, x, y0, alpha, beta), spmv(hip_engine, stream, x, y0, alpha, beta)
            assert same_bits(got, want), (name, alpha, beta)


# ---- 2. / 3. the fused loop ------------------------------------------------------------------------------------------
NIT = 12


def run_loop(hip_engine, s, pre, chunks=((0, NIT),)):
    """BPCG v2 fused loop, tolerance 0, NIT iterations enqueued as `chunks` with a poll() after each"""
    import hipla
    from solvers.bramblepasciak_new import BpcgSession
    f, g = s.rhs(0)
    A, B = hipla.SparseMatrix.from_scipy(s.A), hipla.SparseMatrix.from_scipy(s.B)
    preA = hipla.JacobiPreconditioner(A) if pre == "point" else hipla.BlockJacobi(A, s.line_blocks(3))
    sol = hipla.BlockVector([hipla.Vector(s.n_u), hipla.Vector(s.n_p)])
    with contextlib.redirect_stdout(io.StringIO()):
        ses = BpcgSession(Form(A), Form(B), None, hipla.Vector.from_numpy(f), hipla.Vector.from_numpy(g), preA,
                          hipla.DiagonalMatrix(1.0 / s.mass), sol=sol)
    loop = ses.fused
    ses.first_direction()
    loop.start(ses.wdn, ses.err0, 0.0, True, NIT)
    for a, b in chunks:
        loop.enqueue(a, b)
        loop.poll()
    x = sol.numpy()
    return (loop.history(NIT - 1).copy(), x[:s.n_u].copy(), x[s.n_u:].copy(), ses.matBT.handle.info(),
            loop.c1_applies_preA())


@pytest.fixture(scope="module")
def systems():
    return {(3, 12): mac_stokes(3, 12, 0.01), (2, 40): mac_stokes(2, 40, 0.01)}


@pytest.mark.parametrize("dim,n", [(3, 12), (2, 40)])
@pytest.mark.parametrize("pre,fuse", [("block", 0), ("block", 1), ("point", 0)])
@pytest.mark.parametrize("codes", [0, 1])
@pytest.mark.parametrize("nt", [0, 1])
def test_loop_with_rows_kernel_c1_equals_stream_kernel_c1(hip_engine, systems, dim, n, pre, fuse, codes, nt):
    s = systems[(dim, n)]
    plans = dict(fuse_bjac=fuse, value_codes=codes, block_codes=codes, stream_loads=nt)
    with hip_engine.overrides(direct_rows=-1, **plans):
        stream = run_loop(hip_engine, s, pre)
    with hip_engine.overrides(direct_rows=0, **plans):
        rows = run_loop(hip_engine, s, pre)
    assert rows[3]["operand_form"] == "rows" and stream[3]["operand_form"] != "rows"
    assert rows[3]["value_bytes"] == (1 if codes else 8) * rows[3]["nnz"]
    assert rows[4] == stream[4] == bool(fuse)
    assert np.all(np.isfinite(rows[0])) and rows[0][-1] < rows[0][0]
    for a, b in zip(rows[:3], stream[:3]):
        assert same_bits(a, b)


def test_loop_with_full_row_blocks(hip_engine):
    """1.06e6 velocity rows: B^T has 512-row blocks, so C1 takes the body without a per-lane predicate; in two parts,
    compared with the uninterrupted loop whose C1 is the stream kernel"""
    s = mac_stokes(2, 730, 0.01)
    assert s.n_u > FULL_BLOCK_ROWS
    plans = dict(fuse_bjac=0, value_codes=1, stream_loads=1)
    with hip_engine.overrides(direct_rows=0, **plans):
        rows = run_loop(hip_engine, s, "block", chunks=((0, 5), (5, NIT)))
    assert rows[3]["operand_form"] == "rows" and rows[3]["row_blocks"] >= 2048
    with hip_engine.overrides(direct_rows=-1, **plans):
        stream = run_loop(hip_engine, s, "block")
    assert stream[3]["operand_form"] != "rows"
    assert np.all(np.isfinite(rows[0])) and rows[0][-1] < rows[0][0]
    for a, b in zip(rows[:3], stream[:3]):
        assert same_bits(a, b)


@pytest.mark.parametrize("dim,n", [(3, 12), (2, 40)])
@pytest.mark.parametrize("codes", [0, 1])
def test_loop_in_two_parts_equals_the_uninterrupted_loop(hip_engine, systems, dim, n, codes):
    """(0, 5), poll(), (5, 12): the poll applies the deferred velocity update, so C1 of iteration 5 finds nothing
    pending (its u0 is loaded and not used); iteration 0 takes the body of its own; the last poll flushes."""
    s = systems[(dim, n)]
    plans = dict(fuse_bjac=0, value_codes=codes, stream_loads=1)
    with hip_engine.overrides(direct_rows=0, **plans):
        whole = run_loop(hip_engine, s, "block")
        parts = run_loop(hip_engine, s, "block", chunks=((0, 5), (5, NIT)))
    assert whole[3]["operand_form"] == "rows" and parts[3]["operand_form"] == "rows"
    for a, b in zip(parts[:3], whole[:3]):
        assert same_bits(a, b)
    with hip_engine.overrides(direct_rows=-1, **plans):
        stream = run_loop(hip_engine, s, "block", chunks=((0, 5), (5, NIT)))
    for a, b in zip(parts[:3], stream[:3]):
        assert same_bits(a, b)
