"""Hand-made AMG hierarchies that walk the branches of the joint cycle (csrc/amg.hip: cycle_multi, csr_multi_kernel) and,
with amg_batch = 0, of the single-vector kernels under the same row-block plan: built with a seeded generator for the
kernel's branches, not for multigrid (the cycle is linear and its arithmetic does not care whether the operators are
SPD).  Every row gets a prescribed number of distinct sorted columns, values are +-uniform[0.5, 1.5], level operators
get the diagonal 2 (sum |off-diagonal| + 1), dinv = 1 / diagonal, P and R are independent rectangular matrices.

Each case DECLARES the situations it is made for (`expect`); `check_structure` holds them against the row blocks of the
launch plan that the handles really have, so that a case that stops exercising its branch fails.  Shared by the CPU and
the GPU test; results are computed once per case (callers must not modify them)."""

import functools

import numpy as np
import scipy.sparse as sp

OMEGA = 0.7
MULTI_CHUNK = 1024          # kMultiChunk (csrc/amg.hip): products per row block of the joint cycle's plan
BLOCK = 256                 # kBlock: lanes per workgroup
PREFETCH_SLOTS = 2          # kPF (csr_multi_kernel): pairs per lane group before the tail loop


def multi_lanes(nnz, m):
    """launch_multi (csrc/amg.hip): lanes per (row, component) pair by the mean row length -- thresholds 48 and 20"""
    mean = nnz / m
    return 4 if mean >= 48.0 else (2 if mean >= 20.0 else 1)


def _signed(rng, size):
    return rng.uniform(0.5, 1.5, size) * rng.choice([-1.0, 1.0], size)


def sparse_rows(rng, lengths, ncols, diag=False, palette=None):
    """CSR matrix whose row i has lengths[i] distinct sorted columns; `diag`: square level operator, lengths[i] >= 1
    counts the diagonal, which is 2 (sum |off-diagonal| + 1) (with `palette`: the same constant in every row);
    `palette`: values drawn from these few numbers (a matrix that admits one-byte value codes)"""
    lengths = np.asarray(lengths, dtype=np.int64)
    m = lengths.size
    cols, vals = [], []
    for i, k in enumerate(lengths):
        if diag:
            c = np.sort(rng.choice(ncols - 1, size=k - 1, replace=False)) if k - 1 < ncols - 1 else np.arange(ncols - 1)
            c = np.sort(np.append(c + (c >= i), i))
        else:
            c = np.sort(rng.choice(ncols, size=k, replace=False)) if k < ncols else np.arange(ncols)
        v = _signed(rng, c.size) if palette is None else palette[rng.integers(0, palette.size, c.size)]
        cols.append(c)
        vals.append(v)
    indptr = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int32)
    indices = (np.concatenate(cols) if m else np.zeros(0)).astype(np.int32)
    data = np.concatenate(vals) if m else np.zeros(0)
    mat = sp.csr_matrix((data, indices, indptr), shape=(m, ncols))
    if diag:
        rows = np.repeat(np.arange(m), lengths)
        on = rows == mat.indices
        off = np.bincount(rows[~on], weights=np.abs(mat.data[~on]), minlength=m)
        mat.data[on] = 2.0 * ((off.max() if palette is not None else off) + 1.0)
    return mat


def sparse_rows_many(rng, lengths, ncols, diag=False):
    """sparse_rows for a matrix of very many short rows (at most 8 entries), without a loop over the rows: row i takes
    the columns c, c + o_1, c + o_1 + o_2, ... modulo ncols with random c (`diag`: c = i) and random steps o_j >= 1
    whose sum stays below ncols -- distinct, then sorted"""
    lengths = np.asarray(lengths, dtype=np.int64)
    m, width = lengths.size, int(lengths.max())
    assert 1 <= width <= 8 < ncols
    steps = rng.integers(1, (ncols - 1) // width + 1, (m, width))
    steps[:, 0] = np.arange(m) if diag else rng.integers(0, ncols, m)
    cols = np.cumsum(steps, axis=1) % ncols
    live = np.arange(width)[None, :] < lengths[:, None]
    cols = np.sort(np.where(live, cols, ncols), axis=1)          # (the unused slots last)
    indices = cols[live].astype(np.int32)                         # `live` is a prefix mask: the sorted row's first entries
    indptr = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int32)
    mat = sp.csr_matrix((_signed(rng, indices.size), indices, indptr), shape=(m, ncols))
    if diag:
        rows = np.repeat(np.arange(m), lengths)
        on = rows == mat.indices
        mat.data[on] = 2.0 * (np.bincount(rows[~on], weights=np.abs(mat.data[~on]), minlength=m) + 1.0)
    return mat


def dense_csr(dense):
    """a full matrix as CSR, the arrays written directly (hipla.amg._coarsest)"""
    n = dense.shape[0]
    return sp.csr_matrix((dense.ravel(), np.tile(np.arange(n, dtype=np.int32), n),
                          np.arange(0, n * n + 1, n, dtype=np.int32)), shape=(n, n))


class Hierarchy:
    """`levels`: the non-coarsest levels (dicts A, P, R, dinv); `coarse`: dict A, dinv (unused by the cycle, wanted by
    the handle), inv; `expect`: the declared situations; `coded`: (level, key) of matrices to run through code_values()"""

    def __init__(self, name, levels, coarse, expect=(), coded=()):
        self.name, self.levels, self.coarse, self.omega = name, levels, coarse, OMEGA
        self.expect, self.coded = list(expect), list(coded)
        self.inv = coarse["inv"]
        self.n0 = levels[0]["A"].shape[0] if levels else self.inv.shape[0]

    def matrix(self, where):
        return self.inv if where == "inv" else self.levels[where[0]][where[1]]


def _level(rng, n, nc, a_len, p_len, r_len, **kw):
    A = sparse_rows(rng, a_len, n, diag=True, **kw)
    return dict(A=A, P=sparse_rows(rng, p_len, nc), R=sparse_rows(rng, r_len, n), dinv=1.0 / A.diagonal())


def _coarse(rng, n, inv=None):
    A = sparse_rows(rng, rng.integers(1, min(n, 4) + 1, n), n, diag=True)
    if inv is None:
        inv = dense_csr(_signed(rng, (n, n)) / n)
    return dict(A=A, dinv=1.0 / A.diagonal(), inv=inv)


def _lengths(rng, n, lo, hi, special=None):
    """lo ... hi entries per row, `special` (row -> length) overriding"""
    out = rng.integers(lo, hi + 1, n)
    for r, k in (special or {}).items():
        out[r] = k
    return out


def short_rows():
    """three levels of 65 / 64 / 63 rows, every level operator below 20 entries per row: L = 1, fewer than 8 row blocks"""
    rng = np.random.default_rng(101)
    levels = [_level(rng, 65, 64, _lengths(rng, 65, 3, 7), _lengths(rng, 65, 1, 4), _lengths(rng, 64, 1, 4)),
              _level(rng, 64, 63, _lengths(rng, 64, 3, 7), _lengths(rng, 64, 1, 4), _lengths(rng, 63, 1, 4))]
    expect = [("lanes", (l, k), 1) for l in (0, 1) for k in "APR"] + [("lanes", "inv", 4)]
    expect += [("fewer_than_8_blocks", (l, k)) for l in (0, 1) for k in "APR"] + [("fewer_than_8_blocks", "inv")]
    return Hierarchy("short_rows", levels, _coarse(rng, 63), expect)


def thresholds():
    """level operators with nnz = 20 m, 48 m and one entry short of each: L = 2, 4, 1, 2"""
    rng = np.random.default_rng(102)
    sizes = [304, 303, 302, 301, 37]
    rows = [np.full(304, 20), np.full(303, 48), _lengths(rng, 302, 20, 20, {150: 19}), _lengths(rng, 301, 48, 48, {7: 47})]
    levels = [_level(rng, sizes[l], sizes[l + 1], rows[l], _lengths(rng, sizes[l], 2, 4), _lengths(rng, sizes[l + 1], 2, 4))
              for l in range(4)]
    expect = [("lanes", (0, "A"), 2), ("lanes", (1, "A"), 4), ("lanes", (2, "A"), 1), ("lanes", (3, "A"), 2),
              ("nnz", (0, "A"), 20 * 304), ("nnz", (1, "A"), 48 * 303), ("nnz", (2, "A"), 20 * 302 - 1),
              ("nnz", (3, "A"), 48 * 301 - 1)]
    return Hierarchy("thresholds", levels, _coarse(rng, 37), expect)


def ragged():
    """a few rows of 1024 entries (each a full row block, so that the next block starts behind it) lift the mean row
    length to L = 4 (A, P of level 0) or L = 2 (R of level 0, A of level 1) while most rows have 0 - 2 entries (level
    operators: the diagonal and 0 - 2 more).  The short rows fill row blocks to the plan's row cap: more (row, component)
    pairs than the two prefetch slots per lane group.  (The row behind the last long one is not empty: an empty row
    would join the full block.)"""
    rng = np.random.default_rng(103)
    n0, n1, n2 = 1100, 1050, 40
    long4 = {r: 1024 for r in list(range(30)) + list(range(n0 - 30, n0))}
    long2 = {r: 1024 for r in range(25)}
    levels = [_level(rng, n0, n1, _lengths(rng, n0, 1, 3, long4), _lengths(rng, n0, 0, 2, {**long4, 30: 1}),
                     _lengths(rng, n1, 0, 2, {**long2, 25: 1})),
              _level(rng, n1, n2, _lengths(rng, n1, 1, 3, long2), _lengths(rng, n1, 1, 3), _lengths(rng, n2, 2, 5))]
    expect = [("lanes", (0, "A"), 4), ("lanes", (0, "P"), 4), ("lanes", (0, "R"), 2), ("lanes", (1, "A"), 2),
              ("tail", (0, "A"), 30, 94, 4), ("tail", (0, "P"), 30, 94, 4), ("tail", (0, "R"), 25, 153, 2),
              ("tail", (1, "A"), 25, 153, 2), ("tail", (1, "P"), 0, 256, 1),
              ("block", (0, "A"), 29, 30, 1024), ("block", (0, "P"), 29, 30, 1024), ("block", (0, "R"), 24, 25, 1024)]
    return Hierarchy("ragged", levels, _coarse(rng, n2), expect)


def empty_rows():
    """empty rows in P and R and diagonal-only rows in A at the first and last row of a row block and of the matrix;
    2101 consecutive empty rows of P: whole row blocks without a product"""
    rng = np.random.default_rng(104)
    n0, n1, n2 = 2700, 600, 50

    def holes(n, extra=()):
        return {r: 0 for r in (0, 255, 256, 511, n - 1) + tuple(extra) if r < n}

    def only_diag(n):
        return {r: 1 for r in holes(n)}
    levels = [_level(rng, n0, n1, _lengths(rng, n0, 1, 3, only_diag(n0)),
                     _lengths(rng, n0, 1, 3, holes(n0, range(520, 2621))), _lengths(rng, n1, 1, 3, holes(n1, (300, 301)))),
              _level(rng, n1, n2, _lengths(rng, n1, 1, 3, only_diag(n1)), _lengths(rng, n1, 1, 3, holes(n1, (17,))),
                     _lengths(rng, n2, 1, 3, {0: 0, 25: 0, n2 - 1: 0}))]
    expect = [("block", (0, k), 0, 256, None) for k in "APR"] + [("block", (0, k), 256, 512, None) for k in "APR"]
    expect += [("block", (1, k), 256, 512, None) for k in "AP"]
    expect += [("empty_block", (0, "P"), r, r + 256) for r in range(768, 2560, 256)]
    expect += [("not_a_multiple_of_8_blocks", (0, "A")), ("not_a_multiple_of_8_blocks", (0, "P"))]
    expect += [("empty_row", (0, "R"), 0), ("empty_row", (0, "R"), n1 - 1), ("empty_row", (1, "R"), 0)]
    return Hierarchy("empty_rows", levels, _coarse(rng, n2), expect)


def full_blocks():
    """in A, P and R of level 0: a row of exactly 1024 entries (a full row block), rows of 1023 + 1 entries sharing a
    block, a row of 1025 and one of 3001 entries (blocks of their own: the long-row branch; 3001 is no multiple of 256)"""
    rng = np.random.default_rng(105)
    n0, n1, n2 = 3100, 3050, 45
    special = {0: 1024, 1: 1023, 2: 1, 3: 1025, 4: 3001}
    levels = [_level(rng, n0, n1, _lengths(rng, n0, 2, 4, special), _lengths(rng, n0, 2, 4, special),
                     _lengths(rng, n1, 2, 4, special)),
              _level(rng, n1, n2, _lengths(rng, n1, 2, 4), _lengths(rng, n1, 1, 3), _lengths(rng, n2, 2, 5))]
    expect = []
    for k in "APR":
        expect += [("block", (0, k), 0, 1, 1024), ("block", (0, k), 1, 3, 1024), ("long_row", (0, k), 3, 1025),
                   ("long_row", (0, k), 4, 3001), ("lanes", (0, k), 1)]
    return Hierarchy("full_blocks", levels, _coarse(rng, n2), expect)


def coarse_dense():
    """two levels, 300 -> 1487: the dense coarse inverse of the production size, every row a block of its own"""
    rng = np.random.default_rng(106)
    n0, n1 = 300, 1487
    levels = [_level(rng, n0, n1, _lengths(rng, n0, 3, 7), _lengths(rng, n0, 2, 4), _lengths(rng, n1, 1, 3))]
    expect = [("long_row", "inv", 0, n1), ("long_row", "inv", n1 - 1, n1), ("not_a_multiple_of_8_blocks", "inv"),
              ("lanes", "inv", 4)]
    return Hierarchy("coarse_dense", levels, _coarse(rng, n1), expect)


def coarse_1x1():
    """two levels, 300 -> 1: a coarse level of one row"""
    rng = np.random.default_rng(107)
    levels = [_level(rng, 300, 1, _lengths(rng, 300, 3, 7), _lengths(rng, 300, 0, 1), np.array([120]))]
    coarse = dict(A=sp.csr_matrix(np.array([[4.0]])), dinv=np.array([0.25]), inv=sp.csr_matrix(np.array([[-0.75]])))
    return Hierarchy("coarse_1x1", levels, coarse, [("fewer_than_8_blocks", "inv"), ("fewer_than_8_blocks", (0, "R"))])


def coarse_diagonal():
    """two levels, 300 -> 1487 with a diagonal coarse "inverse" (hipla.amg._coarsest when coarsening stalled)"""
    rng = np.random.default_rng(108)
    n0, n1 = 300, 1487
    levels = [_level(rng, n0, n1, _lengths(rng, n0, 3, 7), _lengths(rng, n0, 2, 4), _lengths(rng, n1, 1, 3))]
    A = sparse_rows(rng, _lengths(rng, n1, 1, 4), n1, diag=True)
    coarse = dict(A=A, dinv=1.0 / A.diagonal(), inv=sp.diags(OMEGA / A.diagonal()).tocsr())
    return Hierarchy("coarse_diagonal", levels, coarse, [("lanes", "inv", 1)])


def coded_level():
    """three levels; A and P of level 0 hold 16 distinct values (and one diagonal value): they admit value codes"""
    rng = np.random.default_rng(109)
    n0, n1, n2 = 700, 200, 30
    palette = _signed(rng, 16)
    A = sparse_rows(rng, _lengths(rng, n0, 3, 7), n0, diag=True, palette=palette)
    P = sparse_rows(rng, _lengths(rng, n0, 1, 4), n1, palette=palette)
    levels = [dict(A=A, P=P, R=sparse_rows(rng, _lengths(rng, n1, 1, 4), n0), dinv=1.0 / A.diagonal()),
              _level(rng, n1, n2, _lengths(rng, n1, 3, 7), _lengths(rng, n1, 1, 3), _lengths(rng, n2, 2, 5))]
    return Hierarchy("coded_level", levels, _coarse(rng, n2), [("distinct_values", (0, "A"), 17), ("distinct_values", (0, "P"), 16)],
                     coded=[(0, "A"), (0, "P")])


def one_level():
    """a hierarchy of the coarse inverse alone (65 rows): components sharing it are cycled one after the other"""
    rng = np.random.default_rng(110)
    return Hierarchy("one_level", [], _coarse(rng, 65))


def many_rows():
    """1 050 000 rows of one or two entries: only from 2 * 256 * 2048 rows on does the launch plan give such a matrix row
    blocks of more than 256 rows (plan_row_blocks, csrc/spmv.hip), and only then do TWO components have more pairs in a
    row block than the prefetch slots of a workgroup"""
    rng = np.random.default_rng(111)
    n0, n1, n2 = 1050000, 700, 30
    A = sparse_rows_many(rng, _lengths(rng, n0, 1, 2), n0, diag=True)
    levels = [dict(A=A, P=sparse_rows_many(rng, _lengths(rng, n0, 0, 2, {0: 1}), n1),
                   R=sparse_rows(rng, _lengths(rng, n1, 1, 3), n0), dinv=1.0 / A.diagonal()),
              _level(rng, n1, n2, _lengths(rng, n1, 3, 7), _lengths(rng, n1, 1, 3), _lengths(rng, n2, 2, 5))]
    expect = [("tail", (0, "A"), 0, 512, 1, "K = 2 too"), ("tail", (0, "P"), 0, 512, 1, "K = 2 too"),
              ("tail", (0, "A"), n0 - n0 % 512, n0, 1, "K = 2 too")]
    return Hierarchy("many_rows", levels, _coarse(rng, n2), expect)


BUILDERS = {f.__name__: f for f in (short_rows, thresholds, ragged, empty_rows, full_blocks, coarse_dense, coarse_1x1,
                                    coarse_diagonal, coded_level)}
NAMES = list(BUILDERS)
LARGE = "many_rows"             # (its own tests: not every property is worth a million rows)
BUILDERS[LARGE] = many_rows


@functools.lru_cache(maxsize=None)
def hierarchy(name):
    return one_level() if name == "one_level" else BUILDERS[name]()


@functools.lru_cache(maxsize=None)
def transform(name, K):
    """T: (n0 + 9) x (K n0) with 3 - 5 entries per row"""
    n0 = hierarchy(name).n0
    rng = np.random.default_rng(1000 + 10 * NAMES.index(name) + K if name in NAMES else 999 + K)
    return (sparse_rows_many if name == LARGE else sparse_rows)(rng, rng.integers(3, 6, n0 + 9), K * n0)


@functools.lru_cache(maxsize=None)
def right_hand_side(n, seed):
    return np.random.default_rng(seed).standard_normal(n)


def check_structure(case, K, row_blocks_of):
    """Hold `case.expect` against the launch plans: `row_blocks_of(where)` gives the first rows of the row blocks of the
    matrix at `where` ((level, key) or "inv") as the handle reports them AFTER the joint cycle's re-plan.  Returns the
    list of the situations found, each naming its row block or mean."""
    found = []
    for item in case.expect:
        kind, where = item[0], item[1]
        mat = case.matrix(where).tocsr()
        rowptr = mat.indptr
        if kind == "lanes":
            mean = mat.nnz / mat.shape[0]
            assert multi_lanes(mat.nnz, mat.shape[0]) == item[2], (case.name, item, mean)
            found.append("%s %s: mean row length %.4f -> L = %d" % (case.name, where, mean, item[2]))
            continue
        if kind == "nnz":
            assert mat.nnz == item[2], (case.name, item, mat.nnz)
            continue
        if kind == "distinct_values":
            assert np.unique(mat.data).size == item[2] <= 256, (case.name, item)
            continue
        if kind == "empty_row":
            assert rowptr[item[2]] == rowptr[item[2] + 1], (case.name, item)
            continue
        blocks = np.asarray(row_blocks_of(where))
        nblk = blocks.size - 1
        assert blocks[0] == 0 and blocks[-1] == mat.shape[0] and np.all(np.diff(blocks) > 0), (case.name, where)
        cnt = rowptr[blocks[1:]] - rowptr[blocks[:-1]]
        # the plan the joint cycle relies on: at most 1024 products per row block, or one row alone
        assert np.all((cnt <= MULTI_CHUNK) | (np.diff(blocks) == 1)), (case.name, where, cnt.max())
        if kind == "fewer_than_8_blocks":
            assert nblk < 8, (case.name, item, nblk)
            found.append("%s %s: %d row blocks" % (case.name, where, nblk))
            continue
        if kind == "not_a_multiple_of_8_blocks":
            assert nblk % 8 != 0, (case.name, item, nblk)
            found.append("%s %s: %d row blocks" % (case.name, where, nblk))
            continue
        r0, r1 = (item[2], item[3]) if kind != "long_row" else (item[2], item[2] + 1)
        at = np.flatnonzero(blocks == r0)
        assert at.size == 1 and blocks[at[0] + 1] == r1, (case.name, item, "no row block [%d, %d)" % (r0, r1), blocks[:12])
        products = int(rowptr[r1] - rowptr[r0])
        if kind == "block":
            assert item[4] is None or products == item[4], (case.name, item, products)
            assert products <= MULTI_CHUNK
        elif kind == "long_row":
            assert products == item[3] > MULTI_CHUNK, (case.name, item, products)
        elif kind == "empty_block":
            assert products == 0 and r1 - r0 > 1, (case.name, item, products)
        elif kind == "tail":
            # more pairs than kPF * kBlock / L: the tail loop runs.  The plan gives a matrix of these sizes row blocks
            # of at most 256 / (lanes per row) rows (plan_row_blocks, csrc/spmv.hip), so with K = 2 the pairs of a block
            # exactly fill the prefetch slots: the boundary, one pair short of the loop (many_rows has the K = 2 loop).
            L = item[4]
            slots = PREFETCH_SLOTS * BLOCK // L
            assert multi_lanes(mat.nnz, mat.shape[0]) == L and products <= MULTI_CHUNK, (case.name, item)
            pairs = (r1 - r0) * K
            assert (pairs > slots) if K == 3 or len(item) > 5 else (pairs == slots), (case.name, item, pairs, slots)
        else:
            raise ValueError(kind)
        found.append("%s %s: row block [%d, %d) with %d products (%s)" % (case.name, where, r0, r1, products, kind))
    return found


def engine_levels(case, engine, storage="fp64", code=True):
    """The level dicts HipEngine.amg_create / NumpyEngine.amg_create take, built on `engine`; returns (levels as applied,
    the fp64 levels).  fp32: own fp32 copies of A, P and R (hipla.amg.stored_levels)."""
    import hipla
    from hipla.amg import stored_levels

    def up(mat):
        return hipla.SparseMatrix.from_scipy(sp.csr_matrix(mat), engine=engine)
    levels = []
    for lv in case.levels:
        levels.append(dict(n=lv["A"].shape[0], A=up(lv["A"]), P=up(lv["P"]), R=up(lv["R"]), dinv=engine.from_host(lv["dinv"])))
    c = case.coarse
    levels.append(dict(n=c["A"].shape[0], A=up(c["A"]), dinv=engine.from_host(c["dinv"]), inv=up(c["inv"])))
    if code and storage == "fp64":
        for l, key in case.coded:
            if hasattr(levels[l][key].handle, "code_values"):
                assert levels[l][key].handle.code_values(), (case.name, l, key)
    return stored_levels(levels, storage), levels


def engine_transform(case_name, K, engine, storage="fp64"):
    """(T, T^T) as applied on `engine`: T^T from CreateTranspose(), both as fp32 copies under fp32 storage"""
    import hipla
    from hipla.matrix import fp32_copy
    T = hipla.SparseMatrix.from_scipy(sp.csr_matrix(transform(case_name, K)), engine=engine)
    TT = T.CreateTranspose()
    return (fp32_copy(T), fp32_copy(TT)) if storage == "fp32" else (T, TT)


def apply(engine, handle, bscale, b, n_out):
    """x = handle(bscale b) on the host; x holds a sentinel before the call: every entry must be written"""
    bb = engine.from_host(b)
    x = engine.zeros(n_out)
    engine.fill(x, 7.25)
    engine.amg_apply(handle, bscale, bb, x)
    engine.synchronize()
    return np.array(engine.to_host(x), copy=True)


def _host_operators(name, storage):
    from amg_cycle_reference import round32_levels
    case = hierarchy(name)
    return (round32_levels(case.levels) if storage == "fp32" else case.levels), case.inv, case.omega


@functools.lru_cache(maxsize=None)
def _transposed(name, K, storage):
    import amg_cycle_reference as ref
    TT = transform(name, K).T.tocsr()
    return ref.round32(TT) if storage == "fp32" else TT


@functools.lru_cache(maxsize=None)
def auxiliary_reference(name, K, storage, bscale, seed):
    """(long-double result, magnitude bound E, tolerance) of T (blockdiag_K cycle) T^T (bscale b), b = right_hand_side"""
    import amg_cycle_reference as ref
    levels, inv, omega = _host_operators(name, storage)
    T = transform(name, K)
    T = ref.round32(T) if storage == "fp32" else T
    TT = _transposed(name, K, storage)
    b = right_hand_side(T.shape[0], seed)
    return (ref.aux_ld(T, K, levels, inv, omega, bscale, b, TT), ref.aux_bound(T, K, levels, inv, omega, bscale, b, TT),
            ref.tolerance(levels, inv, T, TT))


@functools.lru_cache(maxsize=None)
def cycle_reference(name, storage, bscale, seed):
    """the same for the plain handle: bscale V(b)"""
    import amg_cycle_reference as ref
    levels, inv, omega = _host_operators(name, storage)
    b = bscale * right_hand_side(hierarchy(name).n0, seed)
    return ref.cycle_ld(levels, inv, omega, b), ref.cycle_bound(levels, inv, omega, b), ref.tolerance(levels, inv)
