"""Row slots (nss_csr_plan_row_slots): a coded, staged matrix with at most 8 entries per row also holds an eight-slot
copy of its staged positions and value codes, and a row-per-lane kernel (csr_slots_kernel, csr_slots_dual_kernel) keeps
a row's products in registers instead of passing them through LDS.  The products are the same doubles, each rounded on
its own, added in CSR order to 0.0; the lane -> row map and the dot partial per row block are the stream kernel's.  So
every result must be IDENTICAL -- compared on the uint64 views throughout -- to what the stream kernel gives."""

import contextlib
import io

import numpy as np
import pytest
import scipy.sparse as sp

from staggered_grid import mac_stokes

pytestmark = pytest.mark.gpu

# eight column offsets: the runs of a 256-row block are 1000 columns apart (1 and 0 share one), about 1800 staged columns
OFFSETS = np.array([0, 1000, 2000, 3000, 3001, 4000, 5000, 6000])
# six value patterns: both zeros, a negative value, a value that is not a dyadic fraction, a subnormal
VALUES = np.array([-0.0, 0.0, -1.5, 2.0, 1.0 / 3.0, 3.0e-310])


class Form:
    def __init__(self, mat):
        self.mat, self.condense = mat, False


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def offset_rows(rows, offsets, lengths, values, seed):
    """row r holds lengths[r] entries in the columns r + (a random subset of `offsets`), values drawn from `values`"""
    rng = np.random.default_rng(seed)
    rank = np.argsort(np.argsort(rng.random((rows, len(offsets))), axis=1), axis=1)
    mask = rank < np.asarray(lengths)[:, None]
    cols = np.arange(rows)[:, None] + np.asarray(offsets)[None, :]
    indices = cols[mask].astype(np.int32)                               # (row-major: ascending inside a row)
    indptr = np.concatenate([[0], np.cumsum(mask.sum(axis=1))]).astype(np.int32)
    data = np.asarray(values)[rng.integers(0, len(values), size=indices.size)]
    return sp.csr_matrix((data, indices, indptr), shape=(rows, rows + int(np.max(offsets))))


def stencil_like(rows, seed=0):
    rng = np.random.default_rng(100 + seed)
    lengths = rng.integers(0, 9, size=rows)
    if rows >= 3:
        lengths[0], lengths[1] = 0, 8
    else:
        lengths[:] = 5
    mat = offset_rows(rows, OFFSETS, lengths, VALUES, seed)
    if rows >= 3:
        per_row = np.diff(mat.indptr)
        assert per_row.min() == 0 and per_row.max() == 8
    return mat


def many_short_rows():
    """2048 * 512 + 300 rows of 0 - 3 entries (2.4 on average): the launch plan gives row blocks of 512 rows"""
    rows = 2048 * 512 + 300
    lengths = np.random.default_rng(5).choice(4, size=rows, p=[0.05, 0.10, 0.25, 0.60])
    return offset_rows(rows, [0, 1, 2], lengths, VALUES, 6)


def upload(eng, csr):
    csr = sp.csr_matrix(csr)
    return eng.csr_create(csr.shape[0], csr.shape[1], csr.indptr, csr.indices, csr.data)


def spmv(eng, h, x, y0, alpha, beta):
    xb, yb = eng.zeros(h.n), eng.zeros(h.m)
    eng.upload(x, xb)
    eng.upload(y0, yb)
    eng.csr_spmv(h, alpha, xb, beta, yb)
    eng.synchronize()
    return eng.to_host(yb).copy()


def operands(csr, seed=0):
    rng = np.random.default_rng(seed)
    return rng.standard_normal(csr.shape[1]), rng.standard_normal(csr.shape[0])


def twins(eng, mat):
    """(handle with the row slots, handle that refuses them), both coded"""
    with eng.overrides(value_codes=1):
        slots, stream = upload(eng, mat), upload(eng, mat)
        assert slots.code_values() and stream.code_values()
        built = slots.plan_row_slots(1)
        assert not stream.plan_row_slots(0)
    return slots, stream, built


def assert_same_products(eng, a, b, mat, what):
    x, y0 = operands(mat)
    with eng.overrides(value_codes=1):
        for alpha, beta in ((-1.75, 0.625), (1.0, 0.0)):
            assert same_bits(spmv(eng, a, x, y0, alpha, beta), spmv(eng, b, x, y0, alpha, beta)), (what, alpha, beta)


# ---- 1. plain SpMV ------------------------------------------------------------------------------------------------
MATRICES = {
    "stencil_1": lambda: stencil_like(1), "stencil_255": lambda: stencil_like(255), "stencil_256": lambda: stencil_like(256),
    "stencil_257": lambda: stencil_like(257), "stencil_700": lambda: stencil_like(700),
    "mac3d_A": lambda: mac_stokes(3, 12).A, "mac3d_B": lambda: mac_stokes(3, 12).B,
    "mac2d_A": lambda: mac_stokes(2, 40).A, "mac2d_B": lambda: mac_stokes(2, 40).B,
}


@pytest.mark.parametrize("name", sorted(MATRICES))
def test_spmv_with_row_slots_equals_stream_kernel(hip_engine, name):
    mat = sp.csr_matrix(MATRICES[name]())
    slots, stream, built = twins(hip_engine, mat)
    assert built, slots.info()
    info = slots.info()
    assert info["row_slots"] and info["operand_form"] == "staged" and not stream.info()["row_slots"]
    assert info["algorithmic_bytes"] == stream.info()["algorithmic_bytes"]      # (priced as the CSR stream)
    assert_same_products(hip_engine, slots, stream, mat, name)


def test_row_blocks_longer_than_the_workgroup_are_walked_in_pieces(hip_engine):
    mat = many_short_rows()
    assert np.diff(mat.indptr).max() == 3 and np.diff(mat.indptr).min() == 0
    slots, stream, built = twins(hip_engine, mat)
    assert built, slots.info()
    assert np.diff(slots.row_blocks()).max() > 256
    assert_same_products(hip_engine, slots, stream, mat, "pieces")


# ---- 2. refusals ---------------------------------------------------------------------------------------------------
def test_a_row_of_nine_entries_is_refused(hip_engine):
    mat = stencil_like(700).tolil()
    row = 321
    for c in list(OFFSETS) + [3002]:
        mat[row, row + c] = 2.0
    mat = sp.csr_matrix(mat)
    assert np.diff(mat.indptr).max() == 9
    slots, stream, built = twins(hip_engine, mat)
    assert not built and not slots.info()["row_slots"]
    assert_same_products(hip_engine, slots, stream, mat, "nine")


def test_an_uncoded_matrix_is_refused(hip_engine):
    mat = stencil_like(700)
    h = upload(hip_engine, mat)
    assert not h.plan_row_slots(1)                                      # no codes at all
    with hip_engine.overrides(value_codes=0):
        h.code_values()
        assert h.info()["value_bytes"] == 8 * mat.nnz
        assert not h.plan_row_slots(1) and not h.info()["row_slots"]   # codes the kernels do not read


def test_a_replan_drops_the_copy(hip_engine):
    mat = stencil_like(700)
    slots, stream, built = twins(hip_engine, mat)
    assert built
    gen = slots.plan_generation()
    slots.plan_for_pairs()                                              # (runs of ~1800 columns: re-planned, in vain or not)
    assert slots.plan_generation() != gen
    assert not slots.info()["row_slots"]
    assert_same_products(hip_engine, slots, stream, mat, "between")
    with hip_engine.overrides(value_codes=1):
        assert slots.plan_row_slots(-1) is False                        # (-1 builds only what the size rule coded)
        assert slots.plan_row_slots(1) and slots.info()["row_slots"]
    assert_same_products(hip_engine, slots, stream, mat, "again")


# ---- 3. the loop -----------------------------------------------------------------------------------------------------
ITERATIONS = 12


def run_loop(eng, s, pre, slots_a, slots_b, chunks=((0, ITERATIONS),)):
    """(history, u, p, c23_form) of BPCG v2 with the row slots of A / B forced (True) or refused (False)"""
    import hipla
    from solvers.bramblepasciak_new import BpcgSession
    A, B = hipla.SparseMatrix.from_scipy(s.A), hipla.SparseMatrix.from_scipy(s.B)
    preA = hipla.JacobiPreconditioner(A) if pre == "point" else hipla.BlockJacobi(A, s.line_blocks(3))
    f, g = s.rhs(0)
    sol = hipla.BlockVector([hipla.Vector(s.n_u), hipla.Vector(s.n_p)])
    with contextlib.redirect_stdout(io.StringIO()):
        ses = BpcgSession(Form(A), Form(B), None, hipla.Vector.from_numpy(f), hipla.Vector.from_numpy(g), preA,
                          hipla.DiagonalMatrix(1.0 / s.mass), sol=sol)
    loop = ses.fused
    assert loop is not None
    for m, want in ((A, slots_a), (B, slots_b)):
        assert m.handle.info()["value_bytes"] == m.handle.nnz           # (coded: the loop's set-up did it)
        assert m.handle.plan_row_slots(1 if want else 0) == want, m.handle.info()
    ses.first_direction()
    loop.start(ses.wdn, ses.err0, 0.0, True, ITERATIONS)
    form = loop.c23_form()
    for begin, end in chunks:
        loop.enqueue(begin, end)
        done, _, last = loop.poll()
        assert not done and last == end - 1
    x = sol.numpy()
    return loop.history(ITERATIONS - 1).copy(), x[:s.n_u].copy(), x[s.n_u:].copy(), form


VARIANTS = {
    "bjac_apart": ("block", dict(fuse_bjac=0)), "bjac_fused": ("block", dict(fuse_bjac=1)), "point": ("point", dict()),
    "stream_loads_0": ("block", dict(stream_loads=0)), "stream_loads_1": ("block", dict(stream_loads=1)),
}


@pytest.mark.parametrize("dim,n", [(3, 12), (2, 40)])
@pytest.mark.parametrize("variant", sorted(VARIANTS))
def test_loop_with_row_slots_equals_loop_without(hip_engine, dim, n, variant):
    pre, plans = VARIANTS[variant]
    s = mac_stokes(dim, n)
    with hip_engine.overrides(value_codes=1, **plans):
        forced = run_loop(hip_engine, s, pre, True, True)
        refused = run_loop(hip_engine, s, pre, False, False)
    assert forced[3] == 1 and refused[3] == 0
    assert len(forced[0]) == ITERATIONS and np.all(np.isfinite(forced[0])) and forced[0][-1] < forced[0][0]
    for a, b in zip(forced[:3], refused[:3]):
        assert same_bits(a, b)


@pytest.mark.parametrize("dim,n", [(3, 12), (2, 40)])
def test_loop_in_chunks_and_with_slots_on_A_only(hip_engine, dim, n):
    s = mac_stokes(dim, n)
    with hip_engine.overrides(value_codes=1):
        whole = run_loop(hip_engine, s, "block", True, True)
        parts = run_loop(hip_engine, s, "block", True, True, chunks=((0, 5), (5, ITERATIONS)))
        a_only = run_loop(hip_engine, s, "block", True, False)
        refused = run_loop(hip_engine, s, "block", False, False)
    assert whole[3] == 1 and parts[3] == 1 and a_only[3] in (0, 2) and refused[3] == 0
    for other in (parts, a_only, refused):
        for a, b in zip(whole[:3], other[:3]):
            assert same_bits(a, b)
