"""One-byte block codes (nss_bjac_code_blocks): a block-Jacobi handle whose inverse blocks take at most 256 distinct
values -- compared as the 64-bit patterns of the entries the apply kernel reads -- and whose dictionary fits 16 KiB
streams one byte per block; the kernel reads the block from an LDS copy of the dictionary.  The products are the same
doubles times the same operands in the same order, so every result must be IDENTICAL -- compared on the uint64 views
throughout -- to what the uncoded twin of the same handle gives (mode 1 = coded, mode 0 = uncoded)."""

import contextlib
import io
import re

import numpy as np
import pytest
import scipy.sparse as sp

from staggered_grid import mac_stokes

pytestmark = pytest.mark.gpu

DICT_BUDGET = 16 << 10


class Form:
    def __init__(self, mat):
        self.mat, self.condense = mat, False


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def distinct_blocks(bs, count, symmetric, seed=0):
    """`count` well-conditioned bs x bs blocks: SPD, or -- not symmetric -- with an inverse that is not symmetric either"""
    rng = np.random.default_rng(seed)
    out = []
    for k in range(count):
        q = rng.standard_normal((bs, bs))
        blk = (2.0 + k) * np.eye(bs) + 0.5 * (q @ q.T) / bs
        if not symmetric:
            blk = blk + 0.3 * np.triu(rng.standard_normal((bs, bs)), 1) + 0.05 * np.eye(bs) * rng.random()
        out.append(blk)
    return out


def block_system(blocks, pick, extra=0):
    """block-diagonal matrix with blocks[pick[b]] at the dofs b * bs .. b * bs + bs - 1 (then `extra` dofs with a plain
    diagonal), and the table of those runs"""
    bs = blocks[0].shape[0]
    mats = [sp.csr_matrix(blocks[p]) for p in pick] + ([sp.identity(extra, format="csr") * 3.0] if extra else [])
    A = sp.block_diag(mats, format="csr")
    A.sort_indices()
    table = (np.arange(len(pick))[None, :] * bs + np.arange(bs)[:, None]).astype(np.int32)
    return A, table


def jacobi(A, table):
    import hipla
    return hipla.BlockJacobi(hipla.SparseMatrix.from_scipy(sp.csr_matrix(A)), np.ascontiguousarray(table, dtype=np.int32))


def apply_both(eng, handle, n, alpha, beta, seed=1):
    """(y of apply, y of apply_dot, its partials) with the mode in force"""
    rng = np.random.default_rng(seed)
    x, y0 = rng.standard_normal(n), rng.standard_normal(n)
    xb, yb, zb = eng.zeros(n), eng.zeros(n), eng.zeros(n)
    eng.upload(x, xb)
    eng.upload(y0, yb)
    eng.upload(y0, zb)
    eng.bjac_apply(handle, alpha, xb, beta, yb)
    partials = eng.bjac_apply_dot(handle, alpha, xb, zb)
    eng.synchronize()
    return eng.to_host(yb).copy(), eng.to_host(zb).copy(), partials


def assert_twins_agree(eng, handle, n, betas=(0.0, 0.625), alpha=-1.75):
    """stream loads 1: the kernels with the non-temporal loads -- of the code bytes in the coded one -- that the
    automatic mode takes from 20 MiB per vector on (the headline's form); -1: the plain loads of these sizes"""
    for stream_loads in (-1, 1):
        for beta in betas:
            with eng.overrides(stream_loads=stream_loads, block_codes=1):
                coded = apply_both(eng, handle, n, alpha, beta)
            with eng.overrides(stream_loads=stream_loads, block_codes=0):
                plain = apply_both(eng, handle, n, alpha, beta)
            for a, b in zip(coded, plain):
                assert same_bits(a, b), (stream_loads, beta)
            assert np.all(np.isfinite(coded[0])) and np.any(coded[0] != 0.0)
            assert len(coded[2]) == (handle.nblocks + 255) // 256


def stored_doubles(bs, symmetric):
    return bs * (bs + 1) // 2 if symmetric and bs > 1 else bs * bs


# ---- 1. apply bits over block sizes and both stored forms -------------------------------------------------------------
@pytest.mark.parametrize("bs", list(range(1, 17)))
@pytest.mark.parametrize("symmetric", [True, False])
def test_apply_bits_over_block_sizes_and_forms(hip_engine, bs, symmetric):
    blocks = distinct_blocks(bs, 5, symmetric)
    pick = np.random.default_rng(2).integers(0, 5, size=300)
    pick[:5] = np.arange(5)
    A, table = block_system(blocks, pick)
    J = jacobi(A, table)
    d = stored_doubles(bs, symmetric)
    assert 5 * d * 8 <= DICT_BUDGET
    assert J.block_coded and J.handle.block_codes()[0] == 5
    code, dict_ = J.handle.download_block_codes()
    assert dict_.shape == (5, d)                                       # packed form for the symmetric matrix, bs > 1
    assert np.array_equal(code[pick == pick[0]], np.full((pick == pick[0]).sum(), code[0]))
    assert len(np.unique(code)) == 5
    assert_twins_agree(hip_engine, J.handle, A.shape[0])


# ---- 2. index forms and edges -------------------------------------------------------------------------------------------
def test_ragged_line_ends(hip_engine):
    s = mac_stokes(3, 8)
    table = s.line_blocks(3)
    assert np.any(table < 0)                                           # padded blocks
    J = jacobi(s.A, table)
    assert J.block_coded and 1 <= J.handle.block_codes()[0] <= 256
    assert table.shape[1] % 256 != 0
    assert_twins_agree(hip_engine, J.handle, s.n_u)


def test_scattered_dofs_take_the_index_table(hip_engine):
    blocks = distinct_blocks(3, 5, True)
    pick = np.random.default_rng(3).integers(0, 5, size=300)
    A, table = block_system(blocks, pick)
    perm = np.random.default_rng(4).permutation(A.shape[0])            # new position of every dof
    P = sp.csr_matrix((np.ones(perm.size), (perm, np.arange(perm.size))), shape=A.shape)
    A2 = (P @ A @ P.T).tocsr()
    table2 = perm[table].astype(np.int32)
    assert np.any(np.diff(table2, axis=0) != 1)                        # no block is a run: no run words
    J = jacobi(A2, table2)
    assert J.block_coded and J.handle.block_codes()[0] == len(np.unique(pick))
    assert_twins_agree(hip_engine, J.handle, A.shape[0])


def test_uncovered_dofs(hip_engine):
    blocks = distinct_blocks(3, 5, True)
    pick = np.random.default_rng(5).integers(0, 5, size=300)
    A, table = block_system(blocks, pick, extra=37)
    J = jacobi(A, table[:, :290])                                      # the last ten blocks and the extra dofs: in no block
    assert J.block_coded
    assert_twins_agree(hip_engine, J.handle, A.shape[0])
    with hip_engine.overrides(block_codes=1):
        y = apply_both(hip_engine, J.handle, A.shape[0], 2.0, 0.0)[0]
    assert np.all(y[290 * 3:] == 0.0)


@pytest.mark.parametrize("nblocks", [1, 255, 256, 257, 513])
def test_block_counts_around_the_workgroup(hip_engine, nblocks):
    blocks = distinct_blocks(3, 5, True)
    pick = np.random.default_rng(6).integers(0, 5, size=nblocks)
    A, table = block_system(blocks, pick)
    J = jacobi(A, table)
    assert J.block_coded and J.handle.block_codes()[0] == len(np.unique(pick))
    assert_twins_agree(hip_engine, J.handle, A.shape[0])


# ---- 3. refusals ------------------------------------------------------------------------------------------------------
def assert_refused_and_unchanged(eng, J, n):
    assert not J.block_coded and not J.handle.code_blocks()
    n_codes, nbytes = J.handle.block_codes()
    assert n_codes == 0
    with pytest.raises(Exception):
        J.handle.download_block_codes()
    with eng.overrides(block_codes=1):
        forced = apply_both(eng, J.handle, n, -1.75, 0.625)
        assert J.handle.block_codes() == (0, nbytes)
    with eng.overrides(block_codes=0):
        plain = apply_both(eng, J.handle, n, -1.75, 0.625)
    for a, b in zip(forced, plain):
        assert same_bits(a, b)


def test_the_257th_block_is_refused(hip_engine):
    for count in (256, 257):
        blocks = [np.array([[1.0 + k]]) for k in range(count)]         # 1 / (1 + k): all different
        A, table = block_system(blocks, np.arange(count))
        J = jacobi(A, table)
        if count == 256:
            assert J.block_coded and J.handle.block_codes()[0] == 256
            assert_twins_agree(hip_engine, J.handle, A.shape[0])
        else:
            assert_refused_and_unchanged(hip_engine, J, A.shape[0])


def test_a_dictionary_over_the_budget_is_refused(hip_engine):
    blocks = distinct_blocks(16, 40, True)
    assert 40 * stored_doubles(16, True) * 8 > DICT_BUDGET
    A, table = block_system(blocks, np.arange(80) % 40)
    J = jacobi(A, table)
    assert_refused_and_unchanged(hip_engine, J, A.shape[0])
    blocks = distinct_blocks(16, 15, True)                             # 15 x 136 x 8 = 16320 bytes: the largest that fits
    A, table = block_system(blocks, np.arange(80) % 15)
    J = jacobi(A, table)
    assert J.block_coded and J.handle.block_codes()[0] == 15
    assert_twins_agree(hip_engine, J.handle, A.shape[0])
    blocks = distinct_blocks(16, 16, True)                             # 16 x 136 x 8 = 17408 bytes
    A, table = block_system(blocks, np.arange(80) % 16)
    assert_refused_and_unchanged(hip_engine, jacobi(A, table), A.shape[0])


def test_a_gauss_seidel_handle_is_left_alone(hip_engine):
    import hipla
    s = mac_stokes(3, 8)
    A = hipla.SparseMatrix.from_scipy(s.A)
    gs = hipla.BlockGaussSeidel(A, s.line_blocks(3))
    x = hipla.Vector.from_numpy(np.random.default_rng(7).standard_normal(s.n_u))
    before, after = hipla.Vector(s.n_u), hipla.Vector(s.n_u)
    gs.Mult(x, before)
    assert not gs.handle.code_blocks() and gs.handle.block_codes()[0] == 0
    with hip_engine.overrides(block_codes=1):
        gs.Mult(x, after)
    assert same_bits(before.numpy(), after.numpy())


def test_the_sign_of_a_zero_makes_another_block(hip_engine):
    """diag(-2, 4) inverts to [[-0.5, -0.0], [+0.0, 0.25]] (the pivot row is scaled by -0.5); with a (0, 1) entry of two
    denormal steps the elimination leaves fma(tiny, 0.25, -0.0) = +0.0 there and nothing else differs.  A third, plainly
    non-symmetric block keeps the handle in the full-block form, which holds that entry."""
    tiny = 2 * np.nextafter(0.0, 1.0)
    X = np.array([[-2.0, 0.0], [0.0, 4.0]])
    Y = np.array([[-2.0, tiny], [0.0, 4.0]])
    N = np.array([[2.0, 1.0], [0.0, 3.0]])
    mats = [sp.csr_matrix(m) for m in (X, Y, N, X, Y)]
    assert mats[1].nnz == 3
    A = sp.block_diag(mats, format="csr")
    table = (np.arange(5)[None, :] * 2 + np.arange(2)[:, None]).astype(np.int32)
    J = jacobi(A, table)
    assert J.block_coded
    code, dict_ = J.handle.download_block_codes()
    assert dict_.shape == (3, 4) and J.handle.block_codes()[0] == 3
    assert code[0] == code[3] and code[1] == code[4] and len({code[0], code[1], code[2]}) == 3
    x, y = dict_[code[0]], dict_[code[1]]
    assert np.array_equal(x, y) and not same_bits(x, y)                # equal as values, different as patterns
    assert np.signbit(x[1]) and not np.signbit(y[1]) and x[1] == 0.0 and y[1] == 0.0
    assert_twins_agree(hip_engine, J.handle, A.shape[0])


# ---- 4. determinism ---------------------------------------------------------------------------------------------------
def test_two_handles_of_one_matrix_hold_the_same_codes(hip_engine):
    s = mac_stokes(3, 8)
    table = s.line_blocks(3)
    first, second = jacobi(s.A, table), jacobi(s.A, table)
    (c1, d1), (c2, d2) = first.handle.download_block_codes(), second.handle.download_block_codes()
    assert np.array_equal(c1, c2) and same_bits(d1, d2) and d1.shape[1] == 6
    assert len(np.unique(c1)) == d1.shape[0] == first.handle.block_codes()[0]
    assert len({d1[k].tobytes() for k in range(d1.shape[0])}) == d1.shape[0]     # the dictionary holds no block twice


# ---- 5. through the loops -----------------------------------------------------------------------------------------------
def run_loop(s, which, nit=30):
    """(error history, solution) of `nit` iterations with the overrides in force"""
    import hipla
    A, B = hipla.SparseMatrix.from_scipy(s.A), hipla.SparseMatrix.from_scipy(s.B)
    preA, preM = hipla.BlockJacobi(A, s.line_blocks(3)), hipla.DiagonalMatrix(1.0 / s.mass)
    assert preA.block_coded
    f, g = s.rhs(0)
    fv, gv = hipla.Vector.from_numpy(f), hipla.Vector.from_numpy(g)
    out = io.StringIO()
    if which == "bpcg2":
        from solvers.bramblepasciak_new import BramblePasciakCG
        sol = hipla.BlockVector([hipla.Vector(s.n_u), hipla.Vector(s.n_p)])
        with contextlib.redirect_stdout(out):
            BramblePasciakCG(Form(A), Form(B), None, fv, gv, preA, preM, sol, tol=0.0, maxsteps=nit, printrates=True)
        hist = np.array([float(m) for m in re.findall(r"it =\s+\d+\s+err =\s+(\S+)", out.getvalue())])
        return hist, sol.numpy().copy()
    if which == "minres":
        from minres import MinRes
        K = hipla.BlockMatrix([[A, B.T], [B, None]])
        Cm = hipla.BlockMatrix([[preA, None], [None, preM]])
        with contextlib.redirect_stdout(out):
            um, errs = MinRes(mat=K, pre=Cm, rhs=hipla.BlockVector([fv, gv]), maxsteps=nit, tol=1e-30, printrates=False)
        return np.array(errs, dtype=np.float64), um.numpy().copy()
    from bramble_pasciak_cg import bramble_pasciak_cg
    with contextlib.redirect_stdout(out):
        x1, errs1 = bramble_pasciak_cg(A, B, None, preA, preM, fv, gv, tolerance=1e-30, max_steps=nit, print_rates=False)
    return np.array(errs1, dtype=np.float64), x1.numpy().copy()


@pytest.mark.parametrize("dim,n", [(3, 8), (2, 12)])
@pytest.mark.parametrize("which", ["bpcg2", "minres", "bpcg1"])
@pytest.mark.parametrize("stream_loads", [-1, 1])
def test_loops_with_codes_equal_loops_without(hip_engine, dim, n, which, stream_loads):
    """stream_loads 1: the non-temporal forms of the kernels, as at the headline size"""
    s = mac_stokes(dim, n)
    with hip_engine.overrides(fuse_bjac=0, stream_loads=stream_loads):   # BPCG v2: the stand-alone apply runs
        with hip_engine.overrides(block_codes=1):
            coded = run_loop(s, which)
        with hip_engine.overrides(block_codes=0):
            plain = run_loop(s, which)
    assert len(coded[0]) >= 10 and np.all(np.isfinite(coded[0])) and np.all(np.isfinite(coded[1]))
    for a, b in zip(coded, plain):
        assert same_bits(a, b)


# ---- 6. reporting -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["runs-packed", "table-packed", "runs-full", "bs1"])
def test_reported_bytes(hip_engine, case):
    bs = 1 if case == "bs1" else 3
    symmetric = case != "runs-full"
    blocks = distinct_blocks(bs, 5, symmetric)
    pick = np.arange(300) % 5
    A, table = block_system(blocks, pick)
    if case == "table-packed":
        perm = np.random.default_rng(8).permutation(A.shape[0])
        P = sp.csr_matrix((np.ones(perm.size), (perm, np.arange(perm.size))), shape=A.shape)
        A, table = (P @ A @ P.T).tocsr(), perm[table].astype(np.int32)
    J = jacobi(A, table)
    n, nb, d = A.shape[0], 300, stored_doubles(bs, symmetric)
    runs = case != "table-packed"
    before = J.handle.algorithmic_bytes()
    assert before == 8 * nb * bs * bs + 16 * n                          # nss_bjac_info prices the dense blocks in every form
    with hip_engine.overrides(block_codes=1):
        assert J.handle.block_codes() == (5, nb * (1 + (4 if runs else 4 * bs)) + 5 * d * 8 + 16 * n)
    # the stored form: the packed kernel takes the run word, the full-block kernel the index table
    index = 4 if runs and d != bs * bs else 4 * bs
    for mode in (0, -1):                                                # -1, by size: 300 blocks stay uncoded
        with hip_engine.overrides(block_codes=mode):
            assert J.handle.block_codes() == (5, nb * (8 * d + index) + 16 * n)
    assert J.handle.algorithmic_bytes() == before


@pytest.mark.parametrize("mode", [-2, 2])
def test_mode_out_of_range_is_an_error(hip_engine, mode):
    assert hip_engine.lib.nss_bjac_block_code_mode(mode) != 0
    assert b"block_code_mode" in hip_engine.lib.nss_last_error()
