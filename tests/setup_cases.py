"""Seeded inputs for the set-up kernels (csrc/precond.hip: bjac_setup_kernel, bjac_pack_sym_kernel; csrc/amg_setup.hip)
at the branches the grid matrices and scipy.sparse.random never reach.  Every builder returns its inputs together with
`situation`: sentences (what the case is there for) mapped to whether they hold, worked out on the references alone
(setup_reference.py, oracle/krylov_ref.py); the tests assert every one of them.  `figures` are numbers worth printing.

The shapes are the smallest at which each branch is reached."""

import collections

import numpy as np
import scipy.sparse as sp

import setup_reference as sr


def _rng(*key):
    return np.random.default_rng([sum(ord(c) for c in str(k)) * 7919 + len(str(k)) for k in key])


# =====================================================================================================================
# block Jacobi
# =====================================================================================================================
BjacCase = collections.namedtuple("BjacCase", "name A idx n packed run coded singular situation figures")
COUPLING = 1e-3


def _spd(rng, k):
    """q q^T / k + I, the products added column by column (elementwise: the same bits wherever BLAS would differ)"""
    q = rng.standard_normal((k, k))
    return sum(q[:, j, None] * q[None, :, j] for j in range(k)) / k + np.eye(k)


def _orthogonal(rng, k):
    return np.linalg.qr(rng.standard_normal((k, k)))[0]


def _permutation_like(rng, k, noise=1e-3):
    """scaled permutation matrix (a cyclic shift composed with a random permutation of the rest) plus noise"""
    perm = np.roll(np.arange(k), 1 + int(rng.integers(max(k - 1, 1)))) if k > 1 else np.arange(1)
    m = noise * rng.standard_normal((k, k))
    m[np.arange(k), perm] += rng.uniform(0.5, 2.0, k) * rng.choice([-1.0, 1.0], k)
    return m


def system_of_blocks(blocks, rng, layout="runs", uncovered=0, table=None):
    """(A, idx, n): block-diagonal matrix of the dense `blocks` (any sizes) plus weak coupling between neighbouring blocks
    and `uncovered` dofs in no block.  layout "runs": every block a run of consecutive dofs; "shuffled": dofs permuted.
    `table(dof lists) -> idx` builds the index table (default: BlockJacobi._as_table)."""
    from hipla.matrix import BlockJacobi
    sizes = [len(b) for b in blocks]
    n = int(sum(sizes)) + uncovered
    order = rng.permutation(n) if layout == "shuffled" else np.arange(n)
    starts = np.concatenate([[0], np.cumsum(sizes)])
    dofs = [order[starts[k]:starts[k + 1]] for k in range(len(blocks))]
    free = order[starts[-1]:]
    r, c, v = [], [], []
    for d, blk in zip(dofs, blocks):
        blk = np.asarray(blk, dtype=np.float64)
        rr, cc = np.nonzero(blk)                                  # exact zeros of a block are not stored
        r.append(d[rr]), c.append(d[cc]), v.append(blk[rr, cc])
    for a, b in zip(dofs[:-1], dofs[1:]):                         # coupling the gather must leave out
        r.append(np.array([a[0], b[-1]])), c.append(np.array([b[-1], a[0]])), v.append(COUPLING * rng.standard_normal(2))
    for f in free:                                                # dofs in no block: a diagonal entry and a coupling
        r.append(np.array([f, f])), c.append(np.array([f, dofs[0][0]])), v.append(np.array([2.0, COUPLING]))
    A = sp.csr_matrix((np.concatenate(v), (np.concatenate(r), np.concatenate(c))), shape=(n, n))
    A.sort_indices()
    idx = (table or BlockJacobi._as_table)([list(d) for d in dofs])
    return A, idx, n


def _bjac_case(name, A, idx, n, situation, figures=None, singular=0):
    """the facts every block-Jacobi case declares, from the fp64 restatement"""
    inv, bad, piv = sr.block_jacobi_fp64(A, idx)
    bs, nb = idx.shape
    swaps = (piv != np.arange(bs)[None, :]) & ~bad[:, None]
    packed, stored = sr.stored_inverse(inv)
    rel = sr.relative_asymmetry(inv[~bad]) if (~bad).any() else 0.0
    M = sr.gather_blocks(A, idx)
    distinct = len({m.tobytes() for m in M})
    d = bs * (bs + 1) // 2 if packed else bs * bs
    figures = dict(figures or {}, bs=bs, nblocks=nb, blocks_that_swap=int(swaps.any(axis=1).sum()),
                   most_swaps_in_a_block=int(swaps.sum(axis=1).max()), relative_asymmetry=rel, distinct_blocks=distinct)
    situation = dict(situation)
    situation["%d singular block(s)" % singular] = int(bad.sum()) == singular
    if bs > 1 and not singular:                                    # fma must not be able to move the 1e-12 decision
        situation["the symmetry decision is a decade away from 1e-12"] = rel < 0.1 * sr.SYM_TOL or rel > 10 * sr.SYM_TOL
    coded = distinct <= 256 and distinct * d * 8 <= 16384
    case = BjacCase(name, A, idx, n, packed, sr.is_run_table(idx), coded, singular, situation, figures)
    return case, swaps, inv


def swap_2x2(nblocks):
    rng = _rng("swap_2x2", nblocks)
    blocks = []
    for k in range(nblocks):
        a, b = rng.uniform(0.5, 2.0, 2) * rng.choice([-1.0, 1.0], 2)
        blocks.append(np.array([[0.0, a], [b, 0.0]]) if k % 2 == 0 else np.array([[1e-9, 1.0], [1.0, 1.0]]))
    A, idx, n = system_of_blocks(blocks, rng, uncovered=2)
    case, swaps, _ = _bjac_case("swap_2x2[%d]" % nblocks, A, idx, n, {})
    case.situation.update({"every block takes its pivot from row 1 at step 0": bool(swaps[:, 0].all()),
                           "full storage (a != b)": not case.packed, "run table": case.run})
    return case


def saddle(bs, nblocks=48):
    """[[K, g], [g^T, 0]] with K SPD of order bs - 1: a diagonal in [1, 1.5] plus a symmetric perturbation of 0.01 / bs, g with
    magnitudes in [1, 2] -- so that no entry of the inverse K^-1 - K^-1 g g^T K^-1 / s nearly cancels (such an entry is
    asymmetric by rounding alone relative to its own size, and the 1e-12 decision would hang on the order of rounding)"""
    rng = _rng("saddle", bs)
    blocks = []
    for k in range(nblocks):
        S = rng.standard_normal((bs - 1, bs - 1))
        K = np.diag(rng.uniform(1.0, 1.5, bs - 1)) + 0.005 / bs * (S + S.T)
        g = (rng.uniform(1.0, 2.0, bs - 1) * rng.choice([-1.0, 1.0], bs - 1))[:, None]
        blk = np.block([[K, g], [g.T, np.zeros((1, 1))]])
        blocks.append(blk if k % 2 == 0 else blk[::-1, ::-1].copy())          # the zero diagonal entry last / first
    A, idx, n = system_of_blocks(blocks, rng)
    case, swaps, _ = _bjac_case("saddle[%d]" % bs, A, idx, n, {})
    M = sr.gather_blocks(A, idx)
    case.situation.update({"a zero diagonal entry in every block": bool(np.all((np.diagonal(M, axis1=1, axis2=2) == 0).sum(axis=1) == 1)),
                           "symmetric blocks": bool(np.array_equal(M, np.swapaxes(M, 1, 2))),
                           "the blocks with the zero first swap at step 0": bool(swaps[1::2, 0].all()),
                           "packed storage": case.packed})
    return case


def permutation_like(nblocks=40, bs=16):
    rng = _rng("permutation_like")
    A, idx, n = system_of_blocks([_permutation_like(rng, bs) for _ in range(nblocks)], rng, uncovered=3)
    case, swaps, _ = _bjac_case("permutation_like", A, idx, n, {})
    case.situation.update({"every block swaps at more than half of its steps": bool(np.all(swaps.sum(axis=1) > bs // 2)),
                           "full storage": not case.packed})
    return case


def ill_conditioned(bs, nblocks=40):
    rng = _rng("ill_conditioned", bs)
    blocks = [_orthogonal(rng, bs) @ np.diag(np.logspace(0, -10, bs)) @ _orthogonal(rng, bs) for _ in range(nblocks)]
    A, idx, n = system_of_blocks(blocks, rng)
    case, _, _ = _bjac_case("ill_conditioned[%d]" % bs, A, idx, n, {})
    cond = max(np.linalg.cond(b) for b in blocks)
    case.figures["condition"] = cond
    case.situation.update({"condition numbers of 1e10": 5e9 < cond < 2e10, "full storage": not case.packed})
    return case


def pivoted_dense(bs, nblocks=64):
    """non-symmetric blocks with small diagonals, as runs with dofs in no block; bs = 1: scalars"""
    rng = _rng("pivoted_dense", bs)
    blocks = []
    for _ in range(nblocks):
        m = rng.standard_normal((bs, bs))
        m[np.arange(bs), np.arange(bs)] *= 1e-3 if bs > 1 else 1.0
        blocks.append(m)
    A, idx, n = system_of_blocks(blocks, rng, uncovered=5)
    case, swaps, _ = _bjac_case("pivoted_dense[%d]" % bs, A, idx, n, {})
    case.situation.update({"blocks swap" if bs > 1 else "scalar blocks never swap": bool(swaps.any()) == (bs > 1),
                           "full storage": not case.packed, "run table": case.run})
    return case


def ragged_lists():
    """block lists of 1 to 12 dofs through BlockJacobi._as_table, the dofs scattered"""
    rng = _rng("ragged_lists")
    sizes = [1 + k % 12 for k in range(60)]
    A, idx, n = system_of_blocks([_permutation_like(rng, s) for s in sizes], rng, layout="shuffled", uncovered=4)
    case, swaps, _ = _bjac_case("ragged_lists", A, idx, n, {})
    ln = (idx >= 0).sum(axis=0)
    case.situation.update({"blocks of every length from 1 to 12": sorted(set(ln.tolist())) == list(range(1, 13)),
                           "the longer blocks swap": bool(swaps[ln >= 2].any(axis=1).all()),
                           "no run table": not case.run})
    return case


def interior_padding():
    """a prebuilt table whose padding is in the middle of the column (and first, in one block)"""
    rng = _rng("interior_padding")

    def table(dofs):
        idx = -np.ones((5, len(dofs)), dtype=np.int32)
        for b, d in enumerate(dofs):
            slots = [s for s in range(5) if s not in ((1, 3), (2,), (0,))[b % 3]][:len(d)]
            idx[slots, b] = d
        return idx
    sizes = [(3, 4, 4)[b % 3] for b in range(45)]
    A, idx, n = system_of_blocks([_permutation_like(rng, s) for s in sizes], rng, table=table)
    case, swaps, _ = _bjac_case("interior_padding", A, idx, n, {})
    case.situation.update({"a -1 above a dof in every column": bool(np.all([np.any((idx[:-1, b] < 0) & (idx[1:, b] >= 0)) for b in range(idx.shape[1])])),
                           "blocks swap": bool(swaps.any(axis=1).all()), "no run table": not case.run})
    return case


def _one_off(name, eps, bs=5, nblocks=60):
    rng = _rng("one_asymmetric_block")                               # the twins share everything but eps
    blocks = [_spd(rng, bs) for _ in range(nblocks)]
    skew = np.triu(rng.uniform(0.5, 1.0, (bs, bs)), 1)
    blocks[37] = blocks[37] * (1.0 + eps * (skew - skew.T))
    A, idx, n = system_of_blocks(blocks, rng)
    return _bjac_case(name, A, idx, n, {})


def one_asymmetric_block():
    case, _, inv = _one_off("one_asymmetric_block", 1e-6)
    asym = sr.asymmetry(inv)
    case.situation.update({"block 37 alone is asymmetric": asym.tolist() == [b == 37 for b in range(60)],
                           "every block is stored in full": not case.packed})
    return case


def tiny_asymmetry():
    case, _, inv = _one_off("tiny_asymmetry", 1e-14)
    rel = sr.relative_asymmetry(inv[37:38])
    case.figures["asymmetry_of_block_37"] = rel
    case.situation.update({"the inverse of block 37 is asymmetric by about 1e-14": 1e-15 < rel < 1e-13,
                           "packed storage": case.packed})
    return case


def repeated_pivoted():
    rng = _rng("repeated_pivoted")
    kinds = [_permutation_like(rng, 4, noise=0.2) for _ in range(3)]
    A, idx, n = system_of_blocks([kinds[k % 3] for k in range(900)], rng)
    case, swaps, _ = _bjac_case("repeated_pivoted", A, idx, n, {})
    case.situation.update({"three distinct blocks": case.figures["distinct_blocks"] == 3, "every block swaps": bool(swaps.any(axis=1).all()),
                           "full storage": not case.packed, "coded": case.coded})
    return case


def singular_zero_column():
    rng = _rng("singular_zero_column")
    blocks = [_permutation_like(rng, 4, noise=0.3) for _ in range(50)]
    for b, c in ((0, 0), (17, 2), (49, 3)):
        blocks[b][:, c] = 0.0
    A, idx, n = system_of_blocks(blocks, rng)
    return _bjac_case("singular_zero_column", A, idx, n, {}, singular=3)[0]


def singular_after_elimination():
    rng = _rng("singular_after_elimination")
    blocks = [np.array([[5.0, 1.0], [1.0, 3.0]]) + rng.integers(0, 2, (2, 2)) for _ in range(30)]
    blocks[11] = np.array([[1.0, 2.0], [2.0, 4.0]])
    A, idx, n = system_of_blocks(blocks, rng)
    case = _bjac_case("singular_after_elimination", A, idx, n, {}, singular=1)[0]
    M = sr.gather_blocks(A, idx)
    case.situation["no block has a zero column"] = bool(np.all(np.abs(M).sum(axis=1) > 0))
    return case


BJAC_BUILDERS = collections.OrderedDict(
    [("swap_2x2[%d]" % nb, (swap_2x2, nb)) for nb in (1, 255, 256, 257)]
    + [("saddle[%d]" % bs, (saddle, bs)) for bs in (2, 3, 5, 8, 12, 16)]
    + [("permutation_like", (permutation_like,))]
    + [("ill_conditioned[%d]" % bs, (ill_conditioned, bs)) for bs in (8, 16)]
    + [("pivoted_dense[%d]" % bs, (pivoted_dense, bs)) for bs in (1, 3, 5, 12)]
    + [("ragged_lists", (ragged_lists,)), ("interior_padding", (interior_padding,)),
       ("one_asymmetric_block", (one_asymmetric_block,)), ("tiny_asymmetry", (tiny_asymmetry,)),
       ("repeated_pivoted", (repeated_pivoted,))])
BJAC_SINGULAR = collections.OrderedDict([("singular_zero_column", (singular_zero_column,)),
                                         ("singular_after_elimination", (singular_after_elimination,))])
_built = {}


def bjac_case(name):
    if name not in _built:
        f = (BJAC_BUILDERS.get(name) or BJAC_SINGULAR[name])
        _built[name] = f[0](*f[1:])
    return _built[name]


def bjac_vectors(case):
    """two seeded right-hand sides (normal; magnitudes in [0.5, 2] with random signs) and the non-zero y of the MultAdd.
    Entries of one size on purpose: where an inverse has a structural zero (a saddle block), elimination leaves rounding
    noise that E, built on |A_bb|, has no term for, and a right-hand side of wide dynamic range would make the measured
    factor GAMMA a measure of that range."""
    rng = _rng("vectors", case.name)
    return [rng.standard_normal(case.n), rng.uniform(0.5, 2.0, case.n) * rng.choice([-1.0, 1.0], case.n)], rng.standard_normal(case.n)


# =====================================================================================================================
# sparse products
# =====================================================================================================================
SpgemmCase = collections.namedtuple("SpgemmCase", "name X Y integer situation figures")
CAPS = (0, 1, 257)
INT_VALUES = np.array([-2.0, -1.0, 1.0, 2.0])


def _csr(rows, cols, vals, shape):
    m = sp.csr_matrix((np.asarray(vals, dtype=np.float64), (np.asarray(rows), np.asarray(cols))), shape=shape)
    m.sort_indices()
    return m


def _int_csr(rng, m, n, density, empty_rows=()):
    mask = rng.random((m, n)) < density
    mask[list(empty_rows)] = False
    r, c = np.nonzero(mask)
    return _csr(r, c, rng.choice(INT_VALUES, r.size), (m, n))


def structural_pairs(X, Y):
    """number of (i, j) with some k: x_ik and y_kj both stored"""
    ones = lambda M: sp.csr_matrix((np.ones(M.nnz), M.indices, M.indptr), shape=M.shape)
    return int((ones(X) @ ones(Y)).nnz)


def _spgemm_case(name, X, Y, integer, situation):
    from oracle import krylov_ref as kr
    C = kr.sa_spgemm(X, Y)
    lens = np.diff(X.indptr)
    figures = dict(shape="%dx%d times %dx%d" % (X.shape + Y.shape), structural=structural_pairs(X, Y), stored=int(C.nnz),
                   longest_x_row=int(lens.max()) if lens.size else 0, empty_x_rows=int((lens == 0).sum()))
    return SpgemmCase(name, X, Y, integer, dict(situation), figures)


def cancelling():
    rng = _rng("cancelling")
    case = _spgemm_case("cancelling", _int_csr(rng, 64, 48, 0.25), _int_csr(rng, 48, 40, 0.25), True, {})
    case.situation["sums cancel: stored < structural"] = 0 < case.figures["stored"] < case.figures["structural"]
    return case


def row_emptied():
    X = sp.csr_matrix(np.array([[1.0, 1, 0], [0, 0, 1]]))
    Y = sp.csr_matrix(np.array([[3.0, -2], [-3, 2], [0, 0]]))
    case = _spgemm_case("row_emptied", X, Y, True, {})
    case.situation["nnz == 0 with 2 structural pairs"] = case.figures["stored"] == 0 and case.figures["structural"] == 2
    return case


def longest_x_row(length):
    """one row of `length` entries among rows of at most one; empty rows first, last and adjacent"""
    rng = _rng("longest_x_row", length)
    k = 300
    lens = [0, 0, 1, length, 0, 1, 1, 0, 0, 1, 1, 0]
    r = np.repeat(np.arange(len(lens)), lens)
    c = np.concatenate([np.sort(rng.choice(k, n, replace=False)) for n in lens])
    X = _csr(r, c, rng.choice(INT_VALUES, r.size), (len(lens), k))
    Y = _int_csr(rng, k, 37, 0.1, empty_rows=(0, 5, 6, k - 1))
    case = _spgemm_case("longest_x_row[%d]" % length, X, Y, True, {})
    case.situation.update({"longest X row %d" % length: case.figures["longest_x_row"] == length,
                           "empty rows first, last and adjacent": lens[0] == lens[1] == lens[-1] == 0})
    return case


def y_columns(n):
    """Y with n columns and entries in the first and the last of them"""
    rng = _rng("y_columns", n)
    X = _int_csr(rng, 20, 30, 0.3, empty_rows=(3,))
    r = np.repeat(np.arange(30), 3)
    c = np.concatenate([rng.choice(n, min(3, n), replace=False) for _ in range(30)]) if n >= 3 else rng.integers(0, n, 90)
    r = r[:c.size] if n >= 3 else r
    c = np.asarray(c).copy()
    c[0], c[-1], c[c.size // 2] = 0, n - 1, n - 1
    keep = np.unique(np.stack([r[:c.size], c]), axis=1, return_index=True)[1]
    Y = _csr(r[:c.size][keep], c[keep], rng.choice(INT_VALUES, keep.size), (30, n))
    case = _spgemm_case("y_columns[%d]" % n, X, Y, True, {})
    cols = np.unique(Y.indices)
    case.situation["entries in the first and the last of %d columns" % n] = cols[0] == 0 and cols[-1] == n - 1
    return case


def row_count(m):
    rng = _rng("row_count", m)
    case = _spgemm_case("row_count[%d]" % m, _int_csr(rng, m, 20, 0.15), _int_csr(rng, 20, 25, 0.2), True, {})
    case.situation["%d rows" % m] = case.X.shape[0] == m
    return case


def signed_zero():
    """products that underflow to -0.0 and sum to -0.0, next to a sum +x - x = +0.0"""
    t = 1e-200
    X = _csr([0, 0, 1, 2, 2], [0, 1, 2, 0, 2], [-t, -t, 1.0, -t, 1.0], (3, 3))
    Y = _csr([0, 0, 1, 1, 2], [0, 1, 0, 1, 1], [t, 5.0, t, -5.0, 2.0], (3, 2))
    case = _spgemm_case("signed_zero", X, Y, False, {})
    p = np.float64(-t) * np.float64(t)
    case.situation.update({"the products are -0.0 and their sum is": bool(p == 0 and np.signbit(p) and np.signbit(p + p)),
                           "stored < structural": case.figures["stored"] < case.figures["structural"],
                           "2 of 5 pairs stored": (case.figures["stored"], case.figures["structural"]) == (2, 5)})
    return case


SPGEMM_BUILDERS = collections.OrderedDict(
    [("cancelling", (cancelling,)), ("row_emptied", (row_emptied,)), ("signed_zero", (signed_zero,))]
    + [("longest_x_row[%d]" % n, (longest_x_row, n)) for n in (1, 2, 255, 256, 257)]
    + [("y_columns[%d]" % n, (y_columns, n)) for n in (1, 2, 4096, 4097, 65536, 65537)]
    + [("row_count[%d]" % m, (row_count, m)) for m in (1, 255, 256, 257)])


def spgemm_case(name):
    f = SPGEMM_BUILDERS[name]
    return f[0](*f[1:])


# =====================================================================================================================
# transpose
# =====================================================================================================================
TRANSPOSE_SHAPES = ((1000, 1), (1, 5000), (300, 4096), (300, 4097), (50, 65536), (50, 65537))


def transpose_case(m, n):
    """(matrix, situation): a few hot columns (the first and the last among them) hit from many rows; some rows empty"""
    rng = _rng("transpose", m, n)
    hot = np.unique(np.concatenate([[0, n - 1], rng.integers(0, n, 6)]))
    r, c = [], []
    for i in range(m):
        if m > 1 and i % 11 == 3:
            continue
        k = min(n, 2500 if m == 1 else int(rng.integers(1, 5)))
        cols = rng.choice(n, k, replace=False) if m == 1 else np.unique(np.concatenate([rng.choice(hot, min(k, hot.size), replace=False), rng.integers(0, n, 1)]))
        r.append(np.full(cols.size, i)), c.append(cols)
    r, c = np.concatenate(r), np.concatenate(c)
    if m == 1:
        c[:2] = (0, n - 1)
        c = np.unique(c)
        r = r[:c.size]
    M = _csr(r, c, rng.standard_normal(r.size), (m, n))
    counts = np.bincount(M.indices, minlength=n)
    situation = {"entries in the first and the last column": counts[0] > 0 and counts[-1] > 0,
                 "a column hit from many rows": m == 1 or counts.max() >= min(m, 50) // 4}
    return M, situation


# =====================================================================================================================
# aggregation and prolongator
# =====================================================================================================================
AggCase = collections.namedtuple("AggCase", "name A theta priority prolongate situation figures")


def _tridiag(n, lo=-1.0, di=4.0, up=-1.0):
    A = sp.diags([np.full(n - 1, lo), np.full(n, di), np.full(n - 1, up)], [-1, 0, 1]).tocsr()
    A.sort_indices()
    return A


def _agg_case(name, A, theta, priority, prolongate, situation):
    from oracle import krylov_ref as kr
    A = sp.csr_matrix(A)
    A.sort_indices()
    priority = np.asarray(priority, dtype=np.int64)
    g = kr.sa_strength_graph(A, theta)
    agg, nagg = kr.sa_aggregate(A, theta, priority)
    one_sided = int(((g.astype(np.int32) - g.T.tocsr().astype(np.int32)) > 0).sum())      # i -> j strong, j -> i not
    figures = dict(n=A.shape[0], strong_edges=int(g.nnz), one_sided_edges=one_sided, aggregates=nagg,
                   rounds=sr.luby_rounds(g, priority), longest_row=int(np.diff(A.indptr).max()))
    situation = dict(situation)
    situation["priorities distinct and positive"] = priority.min() > 0 and np.unique(priority).size == priority.size
    situation["ids dense"] = np.unique(agg).size == nagg and agg.min() == 0
    return AggCase(name, A, theta, priority, prolongate, situation, figures)


def threshold_tie(above):
    """tridiagonal [-1, 4, -1]: |a_ij| == 0.25 sqrt(4 * 4) exactly"""
    theta = float(np.nextafter(0.25, 1.0)) if above else 0.25
    case = _agg_case("threshold_tie[%s]" % ("above" if above else "at"), _tridiag(10), theta, np.arange(10, 0, -1), True, {})
    case.situation["%d strong edges" % (0 if above else 18)] = case.figures["strong_edges"] == (0 if above else 18)
    return case


def nonsymmetric_strength():
    A = _tridiag(257).tolil()
    for i in range(0, 256, 2):
        A[i, i + 1] = -0.01
    rng = _rng("nonsymmetric_strength")
    case = _agg_case("nonsymmetric_strength", A.tocsr(), 0.25, rng.permutation(257) + 1, True, {})
    case.situation.update({"one-sided strong edges": case.figures["one_sided_edges"] == 128,
                           "strong edges": case.figures["strong_edges"] == 512 - 128})
    return case


def luby_worst_case():
    case = _agg_case("luby_worst_case", _tridiag(257), 0.0, np.arange(1, 258), True, {})
    case.situation.update({"86 aggregates": case.figures["aggregates"] == 86,
                           "about n / 3 rounds": 80 <= case.figures["rounds"] <= 90})
    return case


def star():
    n = 3001
    r = np.concatenate([np.zeros(n - 1, dtype=int), np.arange(1, n), np.arange(n)])
    c = np.concatenate([np.arange(1, n), np.zeros(n - 1, dtype=int), np.arange(n)])
    v = np.concatenate([np.full(2 * (n - 1), -1.0), np.concatenate([[3000.0], np.full(n - 1, 2.0)])])
    rng = _rng("star")
    case = _agg_case("star", _csr(r, c, v, (n, n)), 0.0, rng.permutation(n) + 1, True, {})
    case.situation.update({"one row of 3001 entries": case.figures["longest_row"] == 3001,
                           "one aggregate": case.figures["aggregates"] == 1})
    return case


def components_and_isolated(m):
    """paths of 1 to 7 nodes side by side; the single nodes are diagonal-only rows"""
    rng = _rng("components", m)
    lo, up = np.full(max(m - 1, 0), -1.0), np.full(max(m - 1, 0), -1.0)
    start, k = 0, 0
    while start < m:
        start += 1 + k % 7
        k += 1
        if 0 < start < m:
            lo[start - 1] = up[start - 1] = 0.0
    A = sp.diags([lo, np.full(m, 4.0), up], [-1, 0, 1]).tocsr() if m > 1 else sp.csr_matrix(np.array([[4.0]]))
    A.eliminate_zeros()
    case = _agg_case("components_and_isolated[%d]" % m, A, 0.1, rng.permutation(m) + 1, True, {})
    ncomp = sp.csgraph.connected_components(A, directed=False)[0]
    case.figures["components"] = ncomp
    case.situation.update({"diagonal-only rows": int((np.diff(A.indptr) == 1).sum()) >= 1,
                           "disconnected pieces": ncomp > 1 or m == 1,
                           "no aggregate spans two pieces": case.figures["aggregates"] >= ncomp})
    return case


def no_stored_diagonal():
    A = _tridiag(40).tolil()
    A[17, 17] = 0.0
    A = A.tocsr()
    A.eliminate_zeros()
    rng = _rng("no_stored_diagonal")
    case = _agg_case("no_stored_diagonal", A, 0.6, rng.permutation(40) + 1, False, {})
    from oracle import krylov_ref as kr
    g = kr.sa_strength_graph(A, 0.6)
    case.situation.update({"row 17 has no diagonal entry": 17 not in A.indices[A.indptr[17]:A.indptr[18]],
                           "only the edges at row 17 are strong (theta sqrt(0) = 0)": sorted(zip(*g.nonzero())) == [(16, 17), (17, 16), (17, 18), (18, 17)]})
    return case


AGG_BUILDERS = collections.OrderedDict(
    [("threshold_tie[at]", (threshold_tie, False)), ("threshold_tie[above]", (threshold_tie, True)),
     ("nonsymmetric_strength", (nonsymmetric_strength,)), ("luby_worst_case", (luby_worst_case,)), ("star", (star,)),
     ("no_stored_diagonal", (no_stored_diagonal,))]
    + [("components_and_isolated[%d]" % m, (components_and_isolated, m)) for m in (1, 2, 255, 256, 257)])


def agg_case(name):
    f = AGG_BUILDERS[name]
    return f[0](*f[1:])


ProCase = collections.namedtuple("ProCase", "name A agg nagg omega situation")


def exact_entries():
    from oracle import krylov_ref as kr
    A = sp.csr_matrix(np.array([[2.0, -2, 1, -1], [-2, 2, 0, 0], [1, 0, 4, 0], [-1, 0, 0, 4]]))
    agg = np.array([0, 0, 1, 1], dtype=np.int64)
    P = kr.sa_prolongator(A, agg, 2, 2.0 / 3.0)
    dense = P.toarray()
    situation = {"rows 0 and 1 store exactly 1.0 in column 0 and nothing in column 1":
                 P.indptr[:3].tolist() == [0, 1, 2] and P.indices[:2].tolist() == [0, 0] and P.data[:2].tolist() == [1.0, 1.0],
                 "6 entries": P.nnz == 6, "no stored zero": bool(np.all(P.data != 0)) and dense[0, 1] == 0}
    return ProCase("exact_entries", A, agg, 2, 2.0 / 3.0, situation)


def isolated_unit_omega():
    """omega = 1: an isolated node with diagonal 4.0 gets 1 - 1 * (0.25 * 4) == 0, an empty row of P"""
    from oracle import krylov_ref as kr
    A = _tridiag(9).tolil()
    A[4, 3] = A[3, 4] = A[4, 5] = A[5, 4] = 0.0
    A = A.tocsr()
    A.eliminate_zeros()
    agg = np.array([0, 0, 0, 0, 1, 2, 2, 2, 2], dtype=np.int64)
    P = kr.sa_prolongator(A, agg, 3, 1.0)
    situation = {"row 4 of P is empty": P.indptr[4] == P.indptr[5], "column 1 of P is empty": 1 not in P.indices,
                 "the other rows are not": bool(np.all(np.delete(np.diff(P.indptr), 4) > 0))}
    return ProCase("isolated_unit_omega", A, agg, 3, 1.0, situation)


PRO_BUILDERS = collections.OrderedDict([("exact_entries", exact_entries), ("isolated_unit_omega", isolated_unit_omega)])


# =====================================================================================================================
# csr_permute / csr_select_rows
# =====================================================================================================================
PermuteCase = collections.namedtuple("PermuteCase", "name source rows colmap ncols_out cuts max_rows row_pos index_bytes")
WIDE = 70000


def ragged_source():
    """300 x 300, rows of 0, 1, 7 and 40 entries"""
    rng = _rng("ragged_source")
    lens = np.array([(0, 1, 7, 40)[(r * 7 + r // 4) % 4] for r in range(300)])
    r = np.repeat(np.arange(300), lens)
    c = np.concatenate([np.sort(rng.choice(300, n, replace=False)) for n in lens])
    return _csr(r, c, rng.standard_normal(r.size), (300, 300))


def permute_sources():
    from staggered_grid import mac_stokes
    A = mac_stokes(2, 12).A.tocsr()
    A.sort_indices()
    return collections.OrderedDict([("ragged", ragged_source()), ("stokes", A)])


def _groups(nrows, rng):
    """row_pos of groups of 1 to 12 rows (position of the row in its group), and the group starts"""
    pos, k = [], 0
    while len(pos) < nrows:
        size = 1 + (k * 5 + int(rng.integers(3))) % 12
        pos.extend(range(size))
        k += 1
    pos = np.array(pos[:nrows], dtype=np.uint8)
    return pos, np.flatnonzero(pos == 0)


def permute_cases(source_name, A):
    """the variants of one source: rows (permutation, strict subset, repeats, none) x column map (identity, shuffle inside
    windows of 64, random into 70000 columns) x cuts x max_rows x row_pos"""
    rng = _rng("permute", source_name)
    m, n = A.shape
    perm = rng.permutation(m)
    subset = rng.permutation(m)[: 2 * m // 3]
    repeats = rng.integers(0, m, m + 17)
    ident = np.arange(n)
    local = np.concatenate([a + rng.permutation(min(64, n - a)) for a in range(0, n, 64)])
    wide = rng.choice(WIDE, n, replace=False)
    wide[0], wide[-1] = 0, WIDE - 1                                         # the first and the last output column
    out = []

    def add(tag, rows, colmap, ncols, cuts=None, max_rows=0, grouped=False, index_bytes=None):
        rows = np.asarray(rows, dtype=np.int32)
        pos, starts = _groups(rows.size, rng) if grouped else (None, None)
        if cuts == "middle":                                                # 0, a middle row twice, nrows
            mid = rows.size // 2 if starts is None else int(starts[starts.size // 2])
            cuts = np.array([0, mid, mid, rows.size], dtype=np.int32)
        out.append(PermuteCase("%s-%s" % (source_name, tag), A, rows, colmap.astype(np.int32), ncols,
                               cuts, max_rows, pos, index_bytes))

    add("perm-identity", perm, ident, n, index_bytes=2)
    add("subset-local-cuts-256", subset, local, n, "middle", 256, index_bytes=2)
    add("repeats-wide", repeats, wide, WIDE, index_bytes=4)
    add("perm-wide-cuts-256", perm, wide, WIDE, "middle", 256, index_bytes=4)
    add("perm-identity-groups-5", perm, ident, n, "middle", 5, grouped=True, index_bytes=2)
    add("subset-local-groups-1", subset, local, n, None, 1, grouped=True, index_bytes=2)
    add("repeats-identity-groups-256", repeats, ident, n, "middle", 256, grouped=True, index_bytes=2)
    add("perm-wide-groups-5", perm, wide, WIDE, None, 5, grouped=True)
    add("perm-local-1", perm, local, n, np.array([m], dtype=np.int32), 1, index_bytes=2)
    add("none", np.zeros(0, dtype=np.int32), ident, n, np.array([0], dtype=np.int32), 0)
    return out


def all_permute_cases():
    return [c for name, A in permute_sources().items() for c in permute_cases(name, A)]
