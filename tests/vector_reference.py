"""What the tests of the vector layer share (tests/test_vector_layer_cpu.py, tests/test_vector_kernels_gpu.py): the
launch arithmetic of csrc/blas1.hip restated in Python (never read from the library), the rounding bounds that follow
from the kernels' operation counts, the statements with partly overlapping operands, and a seeded generator of
view-based statements with its long double evaluation.  No GPU, no engine: plain numpy."""

import numpy as np

U = 2.0 ** -53                  # unit roundoff of fp64
LD = np.longdouble
KBLOCK = 256                    # lanes per workgroup
MAX_STREAM_BLOCKS = 65536       # NSS_MAX_STREAM_BLOCKS

# The branch points of the launch arithmetic.  A workgroup has 256 lanes; a lane takes one element, or one double2 in the
# 16-byte forms (so the stride loop then runs over n >> 1 items and lane 0 of workgroup 0 takes the odd tail).
#   fill, lincomb, diag   ceil(n / 1024) workgroups: up to 1024 one trip of the 8-byte loop per 256 elements of ONE
#                         workgroup (n = 257: second trip, 1024: four, 1025: second workgroup); the 16-byte loop trips
#                         at 512 / 513 (n >> 1 = 256 fills the workgroup exactly) and 1024 / 1025
#   dot                   ceil(n / 2048) workgroups: 2047 / 2048 / 2049 and 4097 (third workgroup)
#   gather, reciprocal,   ceil(n / 256) workgroups, one element per lane: 255 / 256 / 257, 511 / 512 / 513, ...
#   upwind flux, triad (8-byte form)
#   triad (16-byte form)  ((n >> 1) + 256) / 256 workgroups, no loop: n = 511 -> 255 items, one workgroup with one idle
#                         lane; 512 -> 256 items, TWO workgroups, the second idle; 513 -> the same plus the tail
#   1, 2, 3               a lone tail, a lone double2, a double2 and a tail
SIZES = (1, 2, 3, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 2047, 2048, 2049, 4097)
DOT_TWO_TRIPS = 524288 + 1      # 257 workgroups -> 257 partial sums: the serial loop of dot_final_kernel runs twice


def gamma(k):
    """k roundings in a row: |fl - exact| <= gamma(k) * (sum of the absolute values of what was rounded)."""
    return k * U / (1.0 - k * U)


def stream_grid(items, per_block):
    return min(max(1, -(-items // per_block)), MAX_STREAM_BLOCKS)


def dot_blocks(n):
    return min(stream_grid(n, KBLOCK * 8), MAX_STREAM_BLOCKS // 2)


def dot_depth(pairs):
    """The largest number of roundings one product x_i y_i passes through on its way into the result of ONE launch of
    launch_dot over `pairs` = [(n, both operands 16-byte aligned), ...]: see test_dot_* for the derivation."""
    total, chain = 0, 0
    for n, vec2 in pairs:
        blocks = dot_blocks(n)
        stride = blocks * KBLOCK
        trips = -(-(n >> 1) // stride) + (n & 1) if vec2 else -(-n // stride)
        chain = max(chain, trips)
        total += blocks
    serial = -(-total // KBLOCK)
    return chain + 1 + 6 + 3 + (serial - 1) + 6 + 3


def two_product(a, b):
    """(p, e) with p = fl(a b) and p + e = a b exactly (Dekker's product over Veltkamp's splitting; numpy never
    contracts, and nothing here comes near over- or underflow)."""
    a, b = np.broadcast_arrays(np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64))
    p = a * b

    def split(v):
        c = 134217729.0 * v                 # 2^27 + 1
        hi = c - (c - v)
        return hi, v - hi

    ah, al = split(a)
    bh, bl = split(b)
    return p, ((ah * bh - p) + ah * bl + al * bh) + al * bl


def dot_reference(pairs):
    """(sum of x . y over `pairs` in long double, sum |x_i y_i|): exact products (two_product), numpy's pairwise long
    double sums -- an error of about log2(n) 2^-64 sum |x_i y_i|, a thousandth of the smallest bound it is held to."""
    total, absum = LD(0), 0.0
    for x, y in pairs:
        p, e = two_product(x, y)
        total += np.sum(p.astype(LD)) + np.sum(e.astype(LD))
        absum += float(np.sum(np.abs(p.astype(LD) + e.astype(LD))))
    return total, absum


def spread(rng, n):
    """Random reals of either sign with magnitudes spread over 1e-3 .. 1e3."""
    return rng.choice([-1.0, 1.0], n) * 10.0 ** rng.uniform(-3.0, 3.0, n)


def small_ints(rng, n):
    return rng.integers(-3, 4, n).astype(np.float64)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


# ---- statements whose plain operand overlaps the destination without being it -------------------------------------------
OVERLAP_N = 4097
OVERLAP_SHIFTS = (1, 2, 64, 256, 1024)


def overlap_statements(n, s):
    """[(name, run(X, Y), ref(x, y))]: `run` executes the statement on two hipla vectors of length n, `ref` on their
    numpy images with the right-hand side formed first.  Destination above the operand ("up") and below it ("down")."""
    lo, hi = slice(0, n - s), slice(s, n)
    out = []
    for tag, d, o in (("up", hi, lo), ("down", lo, hi)):
        def run_copy(X, Y, d=d, o=o):
            X[d].data = X[o]

        def ref_copy(x, y, d=d, o=o):
            x[d] = x[o].copy()

        def run_lin(X, Y, d=d, o=o):
            X[d].data = 2 * X[o] + Y[d]

        def ref_lin(x, y, d=d, o=o):
            x[d] = 2 * x[o] + y[d]

        def run_acc(X, Y, d=d, o=o):
            X[d].data += X[o]

        def ref_acc(x, y, d=d, o=o):
            x[d] = x[d] + x[o]

        out += [("assign-%s-%d" % (tag, s), run_copy, ref_copy), ("lincomb-%s-%d" % (tag, s), run_lin, ref_lin),
                ("accumulate-%s-%d" % (tag, s), run_acc, ref_acc)]
    return out


# ---- seeded view-based statements ----------------------------------------------------------------------------------------
STATEMENT_SIZES = (1, 2, 63, 257, 1025)
_MATRICES = {}


def statement_matrix(n):
    """(scipy CSR, long double dense copy, longest row) of a small random sparse n x n matrix, one per n."""
    import scipy.sparse as sp
    if n not in _MATRICES:
        m = (sp.random(n, n, density=min(1.0, 3.0 / n), random_state=n, format="csr") + sp.identity(n)).tocsr()
        m.sort_indices()
        _MATRICES[n] = (m, m.toarray().astype(LD), int(np.diff(m.indptr).max()))
    return _MATRICES[n]


def pool_length(n):
    return 4 * n + 8


def random_statement(rng, n):
    """(mode, dest, [(coefficient, start, through the matrix)]): destination and operands are the views
    pool[start : start + n] of one pool; a quarter of the operands are the destination itself, a sixth lie 1 .. 3
    elements beside it, the others anywhere (so with 4 n + 8 elements most of them overlap something)."""
    last = pool_length(n) - n
    mode = str(rng.choice(["=", "+=", "-="]))
    dest = int(rng.integers(0, last + 1))
    terms = []
    for _ in range(int(rng.integers(1, 8))):
        kind = rng.random()
        if kind < 0.25:
            start = dest
        elif kind < 0.42:
            start = min(max(dest + int(rng.choice([-3, -2, -1, 1, 2, 3])), 0), last)
        else:
            start = int(rng.integers(0, last + 1))
        terms.append((float(np.float32(rng.uniform(-3.0, 3.0))), start, bool(rng.random() < 0.35)))
    return mode, dest, terms


def run_statement(P, M, n, statement):
    """Execute `statement` on the hipla vector P (the pool) and the hipla matrix M."""
    mode, dest, terms = statement
    expr = None
    for coef, start, with_mat in terms:
        v = P[start:start + n]
        piece = coef * (M * v) if with_mat else coef * v
        expr = piece if expr is None else expr + piece
    D = P[dest:dest + n]
    if mode == "=":
        D.data = expr
    elif mode == "+=":
        D.data += expr
    else:
        D.data -= expr


def statement_reference(pool, n, statement):
    """(new destination in long double, S): the right-hand side formed first from the numpy image `pool`;
    S = sum |c| |x| over the plain terms + sum |c| (|M| |x|) over the matvec terms + |old destination| when the
    statement accumulates -- element-wise, what every launch bound of the statement is a multiple of."""
    mode, dest, terms = statement
    m, dense, _ = statement_matrix(n)
    rhs, S = np.zeros(n, dtype=LD), np.zeros(n)
    for coef, start, with_mat in terms:
        x = pool[start:start + n]
        if with_mat:
            rhs += LD(coef) * (dense @ x.astype(LD))
            S += abs(coef) * (abs(m) @ np.abs(x))
        else:
            rhs += LD(coef) * x.astype(LD)
            S += abs(coef) * np.abs(x)
    old = pool[dest:dest + n]
    if mode == "=":
        return rhs, S
    S += np.abs(old)
    return (old.astype(LD) + rhs if mode == "+=" else old.astype(LD) - rhs), S
