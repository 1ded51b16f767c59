"""References for the device set-up kernels (csrc/precond.hip: bjac_setup_kernel, bjac_pack_sym_kernel; csrc/amg_setup.hip:
nss_csr_permute / nss_csr_transpose and the launch plan they hand to plan_row_blocks), with no engine behind them --
shared by test_setup_reference_cpu.py and test_setup_edges_gpu.py.  The sparse products, the aggregation and the
prolongator have their restatement in oracle/krylov_ref.py (sa_spgemm, sa_aggregate, sa_prolongator).

Block inverses.  The reference is the solve A_bb y_b = x_b in long double (batched Gauss-Jordan with partial pivoting,
np.linalg has no long double); every comparison is componentwise against the magnitude

    E = |A_bb^-1| |A_bb| |A_bb^-1| |x_b|        (long double),    |y - y_ld| <= GAMMA * 2^-53 * E.

`block_jacobi_fp64` restates the kernel in fp64 numpy: same pivot rule (first row of largest |m[r][k]|, strict >), the
row scaled by 1.0 / pivot, the elimination skipped where the factor is exactly 0 -- but without the kernel's fma.

GAMMA is the one measured number.  The largest |err_i| / (2^-53 E_i) of the restatement (inverse by `block_jacobi_fp64`,
storage decision by `stored_inverse`, product by `apply_blocks`) over all non-singular cases of setup_cases.py, two
right-hand sides each, is MEASURED_RATIO = 8.46 (8.453 on tiny_asymmetry, the packed average; 8.32 on permutation_like; below
6.1 elsewhere).  GAMMA = 4 * MEASURED_RATIO = 33.8: room for the kernel's fma and for the packed average.  The injected
faults of test_setup_reference_cpu.py land at 5e8 to 4e17 on the cases they are named for.  The kernel's own largest
ratio on an MI355X is KERNEL_RATIO = 8.51 (tiny_asymmetry; 8.32 on permutation_like), a quarter of GAMMA
(test_setup_edges_gpu.py prints it per case; profiles/setup_edges_tests.md).

E is built on |A_bb|.  Where an inverse has a structural zero (a saddle block [[K, g], [g^T, 0]] inverted without a swap),
elimination leaves rounding noise of the size of its neighbours there, and E has no term for it: against a right-hand
side with entries from 1e-6 to 1e6 the restatement reached a ratio of 1.7e4 on 2 x 2 saddle blocks.  The right-hand sides of
setup_cases.bjac_vectors therefore have entries of one size, and GAMMA measures the elimination, not their range."""

import numpy as np
import scipy.sparse as sp

LD = np.longdouble
U64 = 2.0 ** -53
MEASURED_RATIO = 8.46
GAMMA = 4.0 * MEASURED_RATIO
KERNEL_RATIO = 8.51               # the kernel on an MI355X (recorded from the GPU run, not asserted)
SYM_TOL = 1e-12                   # bjac_pack_sym_kernel


# ---- block inverses ---------------------------------------------------------------------------------------------------
def gather_blocks(A, idx, dtype=np.float64):
    """(nblocks, bs, bs) dense diagonal blocks A_bb of the (bs, nblocks) dof table; a padding slot (-1, anywhere in the
    column) is an identity row and column."""
    idx = np.asarray(idx)
    bs, nb = idx.shape
    coo = sp.csr_matrix(A).tocoo()
    block = -np.ones(A.shape[0], dtype=np.int64)
    slot = np.zeros(A.shape[0], dtype=np.int64)
    cs, bb = np.nonzero(idx >= 0)
    block[idx[cs, bb]], slot[idx[cs, bb]] = bb, cs
    M = np.zeros((nb, bs, bs), dtype=dtype)
    pc, pb = np.nonzero(idx < 0)
    M[pb, pc, pc] = 1
    inside = (block[coo.row] >= 0) & (block[coo.row] == block[coo.col])
    M[block[coo.row[inside]], slot[coo.row[inside]], slot[coo.col[inside]]] = coo.data[inside].astype(dtype)
    return M


def gauss_jordan(M, pivoting=True, swap_left_only=False):
    """Batched Gauss-Jordan on [M | I] in the dtype of M, by the rule of bjac_setup_kernel.  Returns (inverse, singular
    mask, pivot rows (nblocks, bs)); a singular block's inverse is 0.  `pivoting=False` and `swap_left_only=True` are the
    faults test_setup_reference_cpu.py injects."""
    nb, bs, _ = M.shape
    m = np.concatenate([M, np.broadcast_to(np.eye(bs, dtype=M.dtype), M.shape)], axis=2).copy()
    bad = np.zeros(nb, dtype=bool)
    pivots = np.zeros((nb, bs), dtype=np.int64)
    ar = np.arange(nb)
    for k in range(bs):
        piv = k + np.argmax(np.abs(m[:, k:, k]), axis=1) if pivoting else np.full(nb, k)   # argmax: the first maximum
        best = np.abs(m[ar, piv, k])
        bad |= (best == 0) & ~bad
        pivots[:, k] = piv
        width = bs if swap_left_only else 2 * bs
        rows_k, rows_p = m[ar, k, :width].copy(), m[ar, piv, :width].copy()
        m[ar, k, :width], m[ar, piv, :width] = rows_p, rows_k
        with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
            d = M.dtype.type(1) / m[:, k, k]
            m[:, k, :] = m[:, k, :] * d[:, None]
            f = m[:, :, k].copy()
            f[:, k] = 0
            upd = m - f[:, :, None] * m[:, k, None, :]
        m = np.where((f != 0)[:, :, None], upd, m)
        m[bad] = 0                                              # (keeps inf / nan out of the later steps)
    inv = m[:, :, bs:].copy()
    inv[bad] = 0
    return inv, bad, pivots


def block_jacobi_fp64(A, idx, **fault):
    """fp64 restatement of bjac_setup_kernel: (inverse blocks (nblocks, bs, bs), singular mask, pivot rows)."""
    return gauss_jordan(gather_blocks(A, idx, np.float64), **fault)


def asymmetry(inv):
    """per block: whether bjac_pack_sym_kernel counts it (|u - l| > 1e-12 max(|u|, |l|) somewhere)"""
    u, l = inv, np.swapaxes(inv, 1, 2)
    return np.any(np.abs(u - l) > SYM_TOL * np.maximum(np.abs(u), np.abs(l)), axis=(1, 2))


def relative_asymmetry(inv):
    """max over the entries of |u - l| / max(|u|, |l|) (0 where both are 0): how far a case is from the 1e-12 decision"""
    u, l = inv, np.swapaxes(inv, 1, 2)
    big = np.maximum(np.abs(u), np.abs(l))
    return float(np.max(np.where(big > 0, np.abs(u - l) / np.where(big > 0, big, 1), 0.0))) if inv.size else 0.0


def stored_inverse(inv, force_packed=False):
    """(packed?, the blocks the apply kernels multiply with): one asymmetric block makes every block full; otherwise the
    packed average 0.5 (u + l) stands for both triangles.  bs = 1 has no packed form."""
    packed = inv.shape[1] > 1 and (force_packed or not asymmetry(inv).any())
    return packed, (0.5 * (inv + np.swapaxes(inv, 1, 2)) if packed else inv)


def apply_blocks(inv, idx, x, dtype=np.float64):
    """y = sum_b E_b inv_b E_b^T x with the row sums in column order, in `dtype`; dofs in no block stay 0."""
    idx = np.asarray(idx)
    bs, nb = idx.shape
    xb = np.where(idx.T >= 0, np.asarray(x, dtype=dtype)[np.maximum(idx.T, 0)], 0)          # (nb, bs)
    s = np.zeros((nb, bs), dtype=dtype)
    for c in range(bs):
        s = s + inv[:, :, c].astype(dtype) * xb[:, c, None]
    y = np.zeros(len(x), dtype=dtype)
    live = idx.T >= 0
    y[idx.T[live]] = s[live]
    return y


def _ld_inverse(A, idx):
    M = gather_blocks(A, idx, LD)
    inv, bad, _ = gauss_jordan(M)
    if bad.any():
        raise ValueError("%d singular block(s)" % int(bad.sum()))
    return M, inv


def block_solve_ld(A, idx, x):
    """A_bb y_b = x_b for every block, in long double; dofs in no block are 0."""
    _, inv = _ld_inverse(A, idx)
    return apply_blocks(inv, idx, x, LD)


def block_bound(A, idx, x):
    """E = |A_bb^-1| |A_bb| |A_bb^-1| |x_b| in long double; 0 on dofs in no block."""
    M, inv = _ld_inverse(A, idx)
    W = np.abs(inv)
    return apply_blocks(W @ np.abs(M) @ W, idx, np.abs(np.asarray(x, dtype=LD)), LD)


def covered(idx, n):
    mask = np.zeros(n, dtype=bool)
    idx = np.asarray(idx)
    mask[idx[idx >= 0]] = True
    return mask


def is_run_table(idx):
    """every block a run of consecutive dofs with the padding last: the form the handle packs into one word per block"""
    idx = np.asarray(idx)
    bs, nb = idx.shape
    ln = np.where((idx < 0).any(axis=0), np.argmax(idx < 0, axis=0), bs)
    want = np.where(np.arange(bs)[:, None] < ln[None, :], idx[0][None, :] + np.arange(bs)[:, None], -1)
    return bool(np.all(ln > 0) and np.all(idx[0] >= 0) and np.array_equal(np.where(idx < 0, -1, idx), want))


def ratio(got, ref, bound):
    """max_i |got_i - ref_i| / (2^-53 E_i); a component whose bound is 0 must be exact (inf otherwise)"""
    err = np.abs(np.asarray(got, dtype=LD) - ref)
    lim = LD(U64) * bound
    r = np.where(lim > 0, err / np.where(lim > 0, lim, 1), np.where(err > 0, np.inf, 0.0))
    r = np.where(np.isfinite(np.asarray(got, dtype=np.float64)), r, np.inf)
    return float(r.max()) if r.size else 0.0


# ---- permutation and transpose -------------------------------------------------------------------------------------------
def permute_rows_cols(A, rows, colmap, ncols_out):
    """(rowptr, col, val, shape): row r is row rows[r] of A with column c renamed colmap[c]; the entries stay in the
    stored order of the source row (NOT sorted)."""
    A = sp.csr_matrix(A)
    rows = np.asarray(rows, dtype=np.int64)
    colmap = np.asarray(colmap, dtype=np.int64)
    ln = np.diff(A.indptr)[rows] if rows.size else np.zeros(0, dtype=np.int64)
    rowptr = np.concatenate([[0], np.cumsum(ln)]).astype(np.int32)
    src = np.concatenate([np.arange(A.indptr[r], A.indptr[r + 1]) for r in rows] + [np.zeros(0, dtype=np.int64)]).astype(np.int64)
    return rowptr, colmap[A.indices[src]].astype(np.int32), A.data[src].copy(), (rows.size, int(ncols_out))


def as_stored(rowptr, col, val, shape):
    """scipy CSR around the arrays as they are (unsorted rows stay unsorted)"""
    return sp.csr_matrix((np.asarray(val), np.asarray(col), np.asarray(rowptr)), shape=shape)


def transpose_stable(rowptr, col, val, shape):
    """(rowptr, col, val, shape) of the transpose by a stable sort of the entries by column: every row of the result lists
    its source rows ascending (equal source rows -- duplicates -- in stored order)."""
    rowptr, col, val = np.asarray(rowptr), np.asarray(col), np.asarray(val)
    m, n = shape
    src_row = np.repeat(np.arange(m, dtype=np.int32), np.diff(rowptr))
    order = np.argsort(col, kind="stable")
    trow = np.concatenate([[0], np.cumsum(np.bincount(col, minlength=n))]).astype(np.int32)
    return trow, src_row[order], val[order], (n, m)


# ---- launch plan -----------------------------------------------------------------------------------------------------------
def plan_respects(row_blocks, cuts, max_rows, row_pos):
    """None when the launch plan `row_blocks` (first row of every block, then the row count) keeps what nss_csr_permute
    was asked for, else the sentence that says what it breaks:
      - no row block crosses a cut;
      - no block has more than `max_rows` rows (0: no limit), unless it is a single group longer than that;
      - every block boundary is at a row with row_pos == 0 (group start)."""
    rb = np.asarray(row_blocks, dtype=np.int64)
    if rb.size < 1 or rb[0] != 0 or np.any(np.diff(rb) <= 0):
        return "row blocks are not a strictly ascending list from 0"
    nrows = int(rb[-1])
    pos = None if row_pos is None else np.asarray(row_pos)
    if pos is not None and pos.size != nrows:
        return "row_pos has %d entries for %d rows" % (pos.size, nrows)
    for c in ([] if cuts is None else np.asarray(cuts)):
        if 0 < c < nrows and c not in rb:
            return "a row block crosses the cut at %d" % c
    for a, b in zip(rb[:-1], rb[1:]):
        if pos is not None and pos[a] != 0:
            return "the block boundary at row %d splits a group" % a
        if max_rows and b - a > max_rows:
            one_group = pos is not None and not np.any(pos[a + 1:b] == 0)
            if not one_group:
                return "rows %d..%d: %d rows in one block, more than %d" % (a, b, b - a, max_rows)
    return None


# ---- Luby rounds ---------------------------------------------------------------------------------------------------------
def luby_rounds(g, priority):
    """number of rounds of oracle.krylov_ref.sa_mis2 on the strength graph g (the loop nss_amg_aggregate runs)"""
    from oracle import krylov_ref as kr
    cand = np.ones(g.shape[0], dtype=bool)
    rounds = 0
    while cand.any():
        pri = np.where(cand, priority, 0)
        one = kr._neighbour_max(g, pri)
        two = kr._neighbour_max(g, np.maximum(pri, one))
        w = (cand & (pri >= np.maximum(one, two)) & (pri > one)).astype(np.int64)
        near1 = kr._neighbour_max(g, w)
        near2 = kr._neighbour_max(g, np.maximum(w, near1))
        cand &= ~((w > 0) | (near1 > 0) | (near2 > 0))
        rounds += 1
    return rounds
