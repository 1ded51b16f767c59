"""Small matrices that walk the launch ladder of the CSR kernels: one per lanes-per-row value of the launch plan
(1 ... 64, from the mean row length) and at least one per column form (4-byte gather, 16-bit gather, staged), with values
drawn from fewer than 256 distinct doubles so that every one of them admits value codes.  Shared by the coded and the
fp32-storage SpMV walks."""
import numpy as np
import scipy.sparse as sp

CHUNK, BLOCK = 2048, 256


def plan_lanes(mean):
    """plan_row_blocks: the largest power of two for which one reduce pass still covers a full chunk"""
    lanes = 1
    while lanes < 64 and 2 * lanes * (CHUNK // BLOCK) <= mean:
        lanes *= 2
    return lanes


def _values(rng, nnz, distinct=200):
    return rng.standard_normal(distinct)[rng.integers(0, distinct, size=nnz)]


def random_rows(seed, rows, cols, mean):
    """rows of 0.8 ... 1.2 x `mean` entries in sorted random columns of [0, cols)"""
    rng = np.random.default_rng(seed)
    lengths = rng.integers(int(0.8 * mean), int(1.2 * mean) + 1, size=rows)
    indptr = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int32)
    indices = np.concatenate([np.sort(rng.choice(cols, size=k, replace=False)) for k in lengths]).astype(np.int32)
    return sp.csr_matrix((_values(rng, indices.size), indices, indptr), shape=(rows, cols))


def band(seed, rows, diagonals):
    """`diagonals` adjacent diagonals: the interior row length is `diagonals` (prime: no aligned column groups, and the
    shorter rows at both ends rule them out anyway), a row block touches one run of consecutive columns"""
    rng = np.random.default_rng(seed)
    offsets = np.arange(diagonals) - diagonals // 2
    mat = sp.diags([np.ones(rows - abs(o)) for o in offsets], offsets, format="csr")
    mat.sort_indices()
    mat.data = _values(rng, mat.nnz)
    return mat


# (name, builder, lanes per row, operand form): narrow = 40000 columns (10 windows of 4096: 16-bit gather; hundreds of
# runs per row block: not staged), wide = 400000 columns (a row block of ~2000 random entries meets far more than 16
# windows: 4-byte gather)
CASES = [
    ("n7", lambda: random_rows(1, 3000, 40000, 7), 1, "gather16"),
    ("b7", lambda: band(2, 2999, 7), 1, "staged"),
    ("b29", lambda: band(3, 1501, 29), 2, "staged"),
    ("w48", lambda: random_rows(4, 2000, 400000, 48), 4, "gather32"),
    ("n96", lambda: random_rows(5, 1201, 40000, 96), 8, "gather16"),
    ("w190", lambda: random_rows(6, 800, 400000, 190), 16, "gather32"),
    ("b139", lambda: band(7, 803, 139), 16, "staged"),
    ("n380", lambda: random_rows(8, 601, 40000, 380), 32, "gather16"),
    ("w600", lambda: random_rows(9, 600, 400000, 600), 64, "gather32"),
]

