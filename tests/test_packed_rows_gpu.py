"""Packed per-row index words of the BPCG v2 launches (csrc/packed_rows.h):

* the row-slot copy in 20 bytes per row (eight 11-bit staged positions, the length, eight codes) against the same
  kernels over the 24-byte layout (nss_csr_plan_row_slots mode 3);
* 16-bit window-relative columns in the coded fixed-width copy against the same kernel over the 32-bit columns
  (nss_csr_narrow_direct_columns mode 0);
* a uniform diagonal preM taken as one value in C4 against the streamed one (Bpcg2Loop.uniform_diagonal).

Each form only changes how the same indices, codes and doubles reach the same arithmetic, so every comparison is bit
for bit -- on the uint64 views -- against the same library with the form switched off."""

import contextlib
import io

import numpy as np
import pytest
import scipy.sparse as sp

import test_row_slots_gpu as rs
from staggered_grid import mac_stokes

pytestmark = pytest.mark.gpu

same_bits, upload, spmv, operands = rs.same_bits, rs.upload, rs.spmv, rs.operands
SCALINGS = ((-1.75, 0.625), (1.0, 0.0))


def assert_same_products(eng, a, b, mat, what, **plans):
    x, y0 = operands(mat)
    with eng.overrides(value_codes=1, **plans):
        for alpha, beta in SCALINGS:
            assert same_bits(spmv(eng, a, x, y0, alpha, beta), spmv(eng, b, x, y0, alpha, beta)), (what, alpha, beta)


# ---- 1. row slots, plain SpMV ------------------------------------------------------------------------------------------
def slot_twins(eng, mat):
    """(handle with the packed 20-byte rows, handle with the 24-byte rows), both coded"""
    with eng.overrides(value_codes=1):
        packed, wide = upload(eng, mat), upload(eng, mat)
        assert packed.code_values() and wide.code_values()
        assert packed.plan_row_slots(1) and wide.plan_row_slots(3), (packed.info(), wide.info())
        assert packed.info()["row_slot_bytes"] == 20 and wide.info()["row_slot_bytes"] == 24
    return packed, wide


@pytest.mark.parametrize("name", sorted(rs.MATRICES))
def test_spmv_with_packed_rows_equals_wide_rows(hip_engine, name):
    """The stencil-like matrices mix rows of 0 ... 8 entries (asserted where they are built) at 1, 255, 256, 257 and 700
    rows; the grid operators have 5 - 7 (A) and 4 - 6 (B) per row."""
    mat = sp.csr_matrix(rs.MATRICES[name]())
    packed, wide = slot_twins(hip_engine, mat)
    with hip_engine.overrides(value_codes=1):
        info = packed.info()
        assert info["row_slots"] and info["operand_form"] == "staged"
        assert info["algorithmic_bytes"] == wide.info()["algorithmic_bytes"]      # (both priced as the CSR stream)
    assert_same_products(hip_engine, packed, wide, mat, name)


def test_packed_rows_in_row_blocks_walked_in_pieces(hip_engine):
    """Row blocks longer than the workgroup need 2048 x 512 rows: below, the launch plan prefers more, shorter row
    blocks (plan_row_blocks: kMinRowBlocks).  So this is the matrix of the 24-byte form's test, 1.05e6 rows of 0 - 3."""
    mat = rs.many_short_rows()
    packed, wide = slot_twins(hip_engine, mat)
    assert np.diff(packed.row_blocks()).max() > 256
    assert_same_products(hip_engine, packed, wide, mat, "pieces")


def test_a_staged_position_of_2047(hip_engine):
    """256 rows x 8 entries, row r in the columns r + 256 k: ONE row block of 2048 products whose 2048 distinct columns
    form one run of 2048 staged columns -- the most the operand copy holds --, so the staged positions are 0 ... 2047 and
    the last entry of the last row sits at 2047 (0x7ff, all eleven bits)."""
    rows = 256
    lengths = np.full(rows, 8)
    mat = rs.offset_rows(rows, 256 * np.arange(8), lengths, rs.VALUES, 3)
    assert mat.shape == (256, 2048) and np.unique(mat.indices).size == 2048
    packed, wide = slot_twins(hip_engine, mat)
    with hip_engine.overrides(value_codes=1):
        info = packed.info()
    assert info["row_blocks"] == 1 and list(packed.row_blocks()) == [0, 256] and info["nnz"] == 2048
    assert info["operand_form"] == "staged" and info["cols"] == 2048
    assert_same_products(hip_engine, packed, wide, mat, "2047")
    with hip_engine.overrides(value_codes=1):                           # ... and against the stream kernel
        stream = upload(hip_engine, mat)
        assert stream.code_values() and not stream.plan_row_slots(0)
    assert_same_products(hip_engine, packed, stream, mat, "2047 stream")


def test_a_replan_and_a_layout_change_rebuild_the_copy(hip_engine):
    mat = rs.stencil_like(700)
    packed, wide = slot_twins(hip_engine, mat)
    with hip_engine.overrides(value_codes=1):
        assert packed.plan_row_slots(3) and packed.info()["row_slot_bytes"] == 24
        assert packed.plan_row_slots(-1) and packed.info()["row_slot_bytes"] == 24   # (-1 leaves a copy alone)
        assert packed.plan_row_slots(1) and packed.info()["row_slot_bytes"] == 20
        packed.plan_for_pairs()
        assert not packed.info()["row_slots"] and packed.info()["row_slot_bytes"] == 0
        assert packed.plan_row_slots(1) and packed.info()["row_slot_bytes"] == 20
    assert_same_products(hip_engine, packed, wide, mat, "rebuilt")


# ---- 2. 16-bit columns, plain SpMV through the row-per-lane kernel ---------------------------------------------------------
COLUMN_VALUES = np.array([-0.0, 0.0, -1.5, 2.0, 1.0 / 3.0, 3.0e-310, 1.0, -1.0])


def two_per_row(rows, cols, lengths, spread, seed):
    """rows of lengths[r] <= 2 entries in ascending columns within `spread` of r (clipped to the matrix)"""
    rng = np.random.default_rng(seed)
    first = np.minimum(np.arange(rows) + rng.integers(0, spread, size=rows), cols - 2)
    second = np.minimum(first + 1 + rng.integers(0, spread, size=rows), cols - 1)
    lengths = np.asarray(lengths)
    keep = np.stack([lengths >= 1, lengths >= 2], axis=1)
    indices = np.stack([first, second], axis=1)[keep].astype(np.int32)
    indptr = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int32)
    data = COLUMN_VALUES[rng.integers(0, len(COLUMN_VALUES), size=indices.size)]
    return sp.csr_matrix((data, indices, indptr), shape=(rows, cols))


def column_twins(eng, mat, want=True):
    """(handle with the 16-bit columns -- if the matrix admits them --, handle that refuses them), both coded and with
    the fixed-width copy"""
    with eng.overrides(value_codes=1, direct_rows=0):
        narrow, full = upload(eng, mat), upload(eng, mat)
        assert narrow.code_values() and full.code_values()
        assert narrow.info()["operand_form"] == "rows" and full.info()["operand_form"] == "rows"
        assert narrow.info()["direct_columns_16"] == want, narrow.info()     # (built with the codes)
        assert narrow.narrow_direct_columns(1) == want
        assert full.narrow_direct_columns(0) is False and not full.info()["direct_columns_16"]
    return narrow, full


@pytest.mark.parametrize("rows", [1, 2, 255, 256, 257, 511, 512, 513, 1300])
def test_spmv_with_narrow_columns_equals_wide_columns(hip_engine, rows):
    """Rows of 0 / 1 / 2 entries; the first and the last row of every 256-row block, and the matrix's last row, have a
    padding slot (0 or 1 entries, alternating)."""
    lengths = np.random.default_rng(rows).integers(0, 3, size=rows)
    edges = np.unique(np.concatenate([np.arange(0, rows, 256), np.arange(255, rows, 256), [rows - 1]]))
    lengths[edges] = (np.arange(edges.size) + 1) % 2
    mat = two_per_row(rows, rows + 40, lengths, 20, rows)
    narrow, full = column_twins(hip_engine, mat)
    blocks = narrow.row_blocks()
    assert all(lengths[b] < 2 and lengths[e - 1] < 2 for b, e in zip(blocks[:-1], blocks[1:]))
    assert_same_products(hip_engine, narrow, full, mat, rows, direct_rows=0)
    with hip_engine.overrides(value_codes=1):                           # ... and against the stream kernel
        stream = upload(hip_engine, mat)
        assert stream.code_values() and stream.info()["operand_form"] != "rows"
    assert_same_products(hip_engine, narrow, stream, mat, (rows, "stream"), direct_rows=0)


def test_a_row_block_without_a_live_slot(hip_engine):
    rows = 1024
    lengths = np.random.default_rng(1).integers(0, 3, size=rows)
    lengths[256:512] = 0
    mat = two_per_row(rows, rows + 40, lengths, 20, 2)
    narrow, full = column_twins(hip_engine, mat)
    assert list(narrow.row_blocks()) == [0, 256, 512, 768, 1024]
    assert_same_products(hip_engine, narrow, full, mat, "empty block", direct_rows=0)


def test_full_row_blocks_and_a_partial_one(hip_engine):
    """Row blocks of 512 rows -- the form without any per-lane predicate -- need 2048 x 512 rows (plan_row_blocks:
    kMinRowBlocks): 2048 full row blocks and one of 300 rows."""
    rows = 2048 * 512 + 300
    lengths = np.random.default_rng(7).choice(3, size=rows, p=[0.05, 0.15, 0.80])
    mat = two_per_row(rows, rows + 3000, lengths, 1500, 8)
    narrow, full = column_twins(hip_engine, mat)
    sizes = np.diff(narrow.row_blocks())
    assert (sizes == 512).sum() == 2048 and sizes[-1] == 300 and sizes.size == 2049
    assert_same_products(hip_engine, narrow, full, mat, "full blocks", direct_rows=0)


@pytest.mark.parametrize("window,accepted", [(65534, True), (65535, False)])
def test_the_window_limit(hip_engine, window, accepted):
    """One row block whose live columns span exactly `window`: 65534 is taken, 65535 refuses the whole matrix, which then
    gives the same bits through the 32-bit columns."""
    rows, cols = 300, 70000
    mat = two_per_row(rows, cols, np.full(rows, 2), 20, 4)
    lo = int(mat[:256].indices.min())
    mat.indices[mat.indptr[100]:mat.indptr[101]] = [lo, lo + window]   # (every row holds two entries)
    assert np.diff(mat.indptr).min() == 2 and np.diff(mat.indptr).max() == 2
    first = mat[:256]
    assert int(first.indices.max()) - int(first.indices.min()) == window
    narrow, full = column_twins(hip_engine, mat, want=accepted)
    assert list(narrow.row_blocks()) == [0, 256, 300]
    assert_same_products(hip_engine, narrow, full, mat, window, direct_rows=0)
    with hip_engine.overrides(value_codes=1):
        stream = upload(hip_engine, mat)
        assert stream.code_values()
    assert_same_products(hip_engine, narrow, stream, mat, (window, "stream"), direct_rows=0)


def test_a_replan_rebuilds_the_narrow_columns(hip_engine):
    import hipla
    s = mac_stokes(2, 40)
    with hip_engine.overrides(value_codes=1, direct_rows=0, fuse_bjac=1):
        A = hipla.SparseMatrix.from_scipy(s.A)
        BT = hipla.SparseMatrix.from_scipy(s.B.T.tocsr())
        host = s.B.T.tocsr()
        x, y0 = operands(host)
        h = BT.handle
        assert h.code_values() and h.info()["direct_columns_16"]
        want = spmv(hip_engine, h, x, y0, -1.75, 0.625)
        gen = h.plan_generation()
        pre = hipla.BlockJacobi(A, s.line_blocks(2))
        assert h.plan_for_blocks(pre.handle) and h.plan_generation() != gen
        assert h.info()["direct_columns_16"]                           # (new row blocks: new window bases)
        assert same_bits(spmv(hip_engine, h, x, y0, -1.75, 0.625), want)
        h.drop_value_codes()
        assert not h.info()["direct_columns_16"]
        assert same_bits(spmv(hip_engine, h, x, y0, -1.75, 0.625), want)


# ---- 3. the loop -----------------------------------------------------------------------------------------------------
ITERATIONS = 12
FORMS = ("slots", "columns", "diagonal")


def run_loop(eng, s, pre, on):
    """(history, u, p) of BPCG v2 after the sequence (0, 5), poll, (5, 12) with the forms named in `on` in force and the
    others switched off"""
    import hipla
    from solvers.bramblepasciak_new import BpcgSession
    A, B = hipla.SparseMatrix.from_scipy(s.A), hipla.SparseMatrix.from_scipy(s.B)
    preA = hipla.JacobiPreconditioner(A) if pre == "point" else hipla.BlockJacobi(A, s.line_blocks(3))
    f, g = s.rhs(0)
    sol = hipla.BlockVector([hipla.Vector(s.n_u), hipla.Vector(s.n_p)])
    with contextlib.redirect_stdout(io.StringIO()):
        ses = BpcgSession(rs.Form(A), rs.Form(B), None, hipla.Vector.from_numpy(f), hipla.Vector.from_numpy(g), preA,
                          hipla.DiagonalMatrix(1.0 / s.mass), sol=sol)
    loop = ses.fused
    assert loop is not None and loop.value_coded
    BT = loop.keep[2]
    for m in (A, B):
        assert m.handle.plan_row_slots(1 if "slots" in on else 3)
        assert m.handle.info()["row_slot_bytes"] == (20 if "slots" in on else 24)
    assert BT.handle.info()["operand_form"] == "rows"
    assert BT.handle.narrow_direct_columns(1 if "columns" in on else 0) == ("columns" in on)
    loop.uniform_diagonal = "diagonal" in on
    ses.first_direction()
    loop.start(ses.wdn, ses.err0, 0.0, True, ITERATIONS)
    assert loop.c23_form() == 1 and loop.diagonal_by_value() == ("diagonal" in on)
    for begin, end in ((0, 5), (5, ITERATIONS)):
        loop.enqueue(begin, end)
        done, _, last = loop.poll()
        assert not done and last == end - 1
    x = sol.numpy()
    return loop.history(ITERATIONS - 1).copy(), x[:s.n_u].copy(), x[s.n_u:].copy()


@pytest.mark.parametrize("dim,n", [(3, 12), (2, 40)])
@pytest.mark.parametrize("pre,plans", [("block", dict(fuse_bjac=0)), ("point", dict())], ids=["bjac_apart", "point"])
def test_loop_with_each_form_equals_loop_without(hip_engine, dim, n, pre, plans):
    s = mac_stokes(dim, n)
    with hip_engine.overrides(value_codes=1, direct_rows=0, **plans):
        off = run_loop(hip_engine, s, pre, ())
        assert len(off[0]) == ITERATIONS and np.all(np.isfinite(off[0])) and off[0][-1] < off[0][0]
        for on in [(form,) for form in FORMS] + [FORMS]:
            got = run_loop(hip_engine, s, pre, on)
            for a, b in zip(got, off):
                assert same_bits(a, b), on


# ---- 4. the uniform diagonal -------------------------------------------------------------------------------------------
def small_saddle(n_p, seed):
    """a saddle system with n_p pressure dofs, few distinct values (so that the matrices take codes)"""
    rng = np.random.default_rng(seed)
    n_u = 2 * n_p + 3
    A = sp.diags([np.full(n_u - 1, -1.0), np.full(n_u, 4.0), np.full(n_u - 1, -1.0)], [-1, 0, 1], format="csr")
    rows = np.repeat(np.arange(n_p), 2)
    cols = (2 * np.arange(n_p)[:, None] + np.array([0, 3])[None, :]).ravel()
    B = sp.csr_matrix((np.tile([1.0, -1.0], n_p), (rows, cols)), shape=(n_p, n_u))
    return A, B, rng.standard_normal(n_u), np.zeros(n_p)


def diagonal_session(eng, n_p, diag):
    import hipla
    from solvers.bramblepasciak_new import BpcgSession
    A, B, f, g = small_saddle(n_p, n_p)
    hA, hB = hipla.SparseMatrix.from_scipy(A), hipla.SparseMatrix.from_scipy(B)
    sol = hipla.BlockVector([hipla.Vector(A.shape[0]), hipla.Vector(n_p)])
    with contextlib.redirect_stdout(io.StringIO()):
        ses = BpcgSession(rs.Form(hA), rs.Form(hB), None, hipla.Vector.from_numpy(f), hipla.Vector.from_numpy(g),
                          hipla.JacobiPreconditioner(hA), hipla.DiagonalMatrix(diag), sol=sol)
    assert ses.fused is not None
    return ses, sol


def run_diagonal(eng, n_p, diag, by_value, steps=3):
    ses, sol = diagonal_session(eng, n_p, diag)
    loop = ses.fused
    loop.uniform_diagonal = by_value
    ses.first_direction()
    loop.start(ses.wdn, ses.err0, 0.0, True, steps)
    taken = loop.diagonal_by_value()
    loop.enqueue(0, steps)
    loop.poll()
    return loop.history(steps - 1).copy(), sol.numpy().copy(), taken


@pytest.mark.parametrize("n_p", [1, 2, 511, 512, 513])
def test_uniform_diagonal_by_value_equals_streamed(hip_engine, n_p):
    """n_p = 1 and odd n_p end in the scalar tail of the double2 path; 512 / 513 are one workgroup and one more."""
    value = 0.3
    with hip_engine.overrides(value_codes=1):
        uniform = np.full(n_p, value)
        streamed = run_diagonal(hip_engine, n_p, uniform, False)
        by_value = run_diagonal(hip_engine, n_p, uniform, True)
        assert by_value[2] and not streamed[2]
        assert np.all(np.isfinite(streamed[0])) and same_bits(by_value[0], streamed[0]) and same_bits(by_value[1], streamed[1])
        # one entry one ulp off: not uniform, the diagonal is streamed -- and gives what it gives with the form off
        # (a single entry is uniform whatever its value)
        for where in sorted({0, n_p // 2, n_p - 1}) if n_p > 1 else ():
            off = uniform.copy()
            off[where] = np.nextafter(value, 1.0)
            got, want = run_diagonal(hip_engine, n_p, off, True), run_diagonal(hip_engine, n_p, off, False)
            assert not got[2]
            assert same_bits(got[0], want[0]) and same_bits(got[1], want[1])


def test_detection_looks_at_the_bit_patterns_at_every_start(hip_engine):
    n_p = 513
    with hip_engine.overrides(value_codes=1):
        ses, _ = diagonal_session(hip_engine, n_p, np.full(n_p, 0.3))
        loop = ses.fused
        loop.uniform_diagonal = True
        ses.first_direction()

        def starts_with(diag):
            hip_engine.upload(np.ascontiguousarray(diag, dtype=np.float64), loop.minv)
            loop.start(ses.wdn, ses.err0, 0.0, True, 4)
            return loop.diagonal_by_value()

        assert starts_with(np.full(n_p, 0.3))
        one_ulp = np.full(n_p, 0.3)
        one_ulp[n_p - 1] = np.nextafter(0.3, 0.0)
        assert not starts_with(one_ulp)                                 # a second start, another diagonal: looked at afresh
        assert starts_with(np.full(n_p, 0.25))
        zeros = np.zeros(n_p)
        assert starts_with(zeros)
        zeros[7] = -0.0
        assert not starts_with(zeros)                                   # -0.0 among +0.0: another pattern
        assert starts_with(np.full(n_p, -0.0))
        loop.uniform_diagonal = False
        assert not starts_with(np.full(n_p, 0.3))
