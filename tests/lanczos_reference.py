"""Reference code of the single-step Lanczos tests (tests/test_lanczos_reference_cpu.py, tests/test_lanczos_steps_gpu.py):
the preconditioned Lanczos recurrence of oracle/krylov_ref.py::lanczos_ritz on dense arrays in any precision, the
un-normalised form csrc/lanczos.hip runs, operators and block covers no grid produces, and a case in which every
operation of the loop is exact.  Nothing here touches the package's engine."""

import collections
import functools

import numpy as np
import scipy.sparse as sp

LD = np.longdouble
BREAKDOWN = 1e-14                 # gamma_{j+1} <= BREAKDOWN max(|delta_0|, |delta_j|): the loop's rule

# hist[j] = (delta_j, gamma_{j+1}); rh, zh = gamma_J v_J, gamma_J z_J after the last step made (the device's
# un-normalised vectors); breakdown = the step at which the rule fired (None: none, -1: gamma_0 == 0)
Result = collections.namedtuple("Result", "hist rh zh breakdown")


# ---- preconditioners ------------------------------------------------------------------------------------------------
def table(blocks):
    """(bs, nblocks) int32 table of a list of dof lists, -1 = padding (the form oracle.krylov_ref.block_jacobi takes)."""
    bs = max(len(b) for b in blocks)
    tab = -np.ones((bs, len(blocks)), dtype=np.int32)
    for k, b in enumerate(blocks):
        tab[: len(b), k] = b
    return tab


class BlockInverse:
    """P = scale * sum_b E_b X_b E_b^T with X_b the inverse of A's diagonal block over the dofs `blocks[b]` in long
    double: inverted in float64, then refined by Newton steps X += X (I - M X).  Dofs in no block map to zero.
    ``P @ x`` applies it in the precision it was cast to (`astype`)."""

    def __init__(self, A, blocks, scale=1.0):
        A = np.asarray(A, dtype=np.float64)
        self.n = A.shape[0]
        self.tab = table(blocks)
        bs, nb = self.tab.shape
        self.inv = np.zeros((nb, bs, bs), dtype=LD)
        for k, dofs in enumerate(blocks):
            M = A[np.ix_(dofs, dofs)].astype(LD)
            X = np.linalg.inv(M.astype(np.float64)).astype(LD)
            eye = np.eye(len(dofs), dtype=LD)
            for _ in range(3):
                X = X + X @ (eye - M @ X)
            self.inv[k, : len(dofs), : len(dofs)] = X
        self.scale = scale
        self.dtype = LD

    def astype(self, dtype):
        out = object.__new__(BlockInverse)
        out.__dict__.update(self.__dict__)
        out.inv, out.dtype = self.inv.astype(dtype), dtype
        return out

    def scaled(self, scale):
        out = self.astype(self.dtype)
        out.scale = self.scale * scale
        return out

    def __matmul__(self, x):
        live, safe = self.tab >= 0, np.maximum(self.tab, 0)
        xb = np.where(live, x[safe], 0)
        yb = np.einsum("krc,ck->rk", self.inv, xb)
        y = np.zeros(self.n, dtype=self.dtype)
        y[self.tab[live]] = yb[live]
        return y * self.dtype(self.scale) if self.scale != 1.0 else y

    def dense(self):
        return np.stack([self @ e for e in np.eye(self.n, dtype=self.dtype)], axis=1)

    def covered(self):
        mask = np.zeros(self.n, dtype=bool)
        mask[self.tab[self.tab >= 0]] = True
        return mask


def point_jacobi(A, scale=1.0):
    return BlockInverse(A, [[i] for i in range(np.shape(A)[0])], scale)


# ---- the recurrences ------------------------------------------------------------------------------------------------
def recurrence(A, P, start, steps, dtype=LD):
    """The normalised recurrence of oracle.krylov_ref.lanczos_ritz, statement by statement, in `dtype`: `A` a dense
    array, `P` a `BlockInverse` (or anything with ``@`` and ``astype``)."""
    A, P = np.asarray(A).astype(dtype), P.astype(dtype)
    v = np.asarray(start).astype(dtype)
    v_old = np.zeros_like(v)
    z = P @ v
    gamma = np.sqrt(abs(z @ v))
    if gamma == 0:
        return Result(np.zeros((0, 2), dtype=dtype), v, z, -1)
    rh, zh = v, z
    z = z / gamma
    v = v / gamma
    hist, breakdown, scale0 = [], None, None
    for j in range(steps):
        p = A @ z
        delta = p @ z
        v_new = p - delta * v - gamma * v_old
        z_new = P @ v_new
        gamma_new = np.sqrt(abs(z_new @ v_new))
        hist.append((delta, gamma_new))
        rh, zh = v_new, z_new
        if scale0 is None:
            scale0 = abs(delta)
        if gamma_new <= BREAKDOWN * max(scale0, abs(delta)):
            breakdown = j
            break
        z_new = z_new / gamma_new
        v_new = v_new / gamma_new
        v_old, v = v, v_new
        z = z_new
        gamma = gamma_new
    return Result(np.array(hist, dtype=dtype).reshape(-1, 2), rh, zh, breakdown)


def device_form(A, P, start, steps):
    """The un-normalised recurrence of the header comment of csrc/lanczos.hip in float64 numpy: rh_j = gamma_j v_j and
    zh_j = gamma_j z_j are carried, the factors go into the coefficients."""
    A, P = np.asarray(A, dtype=np.float64), P.astype(np.float64)
    rh = np.asarray(start, dtype=np.float64).copy()
    rh_old = np.zeros_like(rh)
    zh = P @ rh
    gamma = np.sqrt(abs(zh @ rh))
    if gamma == 0.0:
        return Result(np.zeros((0, 2)), rh, zh, -1)
    hist, breakdown, scale0, gamma_old = [], None, None, None
    for j in range(steps):
        ph = A @ zh
        delta = (ph @ zh) / (gamma * gamma)
        ca, cb = 1.0 / gamma, -delta / gamma
        rh_new = ca * ph + cb * rh
        if j > 0:
            rh_new = rh_new + (-gamma / gamma_old) * rh_old
        zh_new = P @ rh_new
        gamma_new = np.sqrt(abs(zh_new @ rh_new))
        hist.append((delta, gamma_new))
        rh_old, rh, zh = rh, rh_new, zh_new
        gamma_old, gamma = gamma, gamma_new
        if scale0 is None:
            scale0 = abs(delta)
        if gamma_new <= BREAKDOWN * max(scale0, abs(delta)):
            breakdown = j
            break
    return Result(np.array(hist).reshape(-1, 2), rh, zh, breakdown)


# ---- operators and covers -------------------------------------------------------------------------------------------
def spd(n, seed, coupling=0.6):
    """A = diag(d) + coupling R / |R|_inf (scipy CSR): d uniform in [1, 2]; R = S + S^T with 0 to 5 entries drawn per
    row of S, and the rows i = 3 (mod 8) neither drawing nor drawn, so an eighth of the rows of R is empty.  Strictly
    diagonally dominant, hence positive definite, with the spectrum of D^-1 A inside [1 - coupling, 1 + coupling]."""
    rng = np.random.default_rng(seed)
    d = 1.0 + rng.random(n)
    open_rows = np.array([i for i in range(n) if i % 8 != 3], dtype=np.int64)
    rows, cols, vals = [], [], []
    for i in open_rows:
        others = open_rows[open_rows != i]
        k = min(int(rng.integers(0, 6)), others.size)
        for c in rng.choice(others, size=k, replace=False):
            rows.append(i)
            cols.append(int(c))
            vals.append(rng.standard_normal())
    S = sp.csr_matrix((vals, (rows, cols)), shape=(n, n))
    R = (S + S.T).tocsr()
    norm = abs(R).sum(axis=1).max() if R.nnz else 0.0
    A = sp.diags(d).tocsr() if norm == 0.0 else (sp.diags(d) + (coupling / norm) * R).tocsr()
    A.sort_indices()
    return A


def ragged_runs(n, bs, seed):
    """Blocks that are runs of consecutive dofs and together cover 0 .. n - 1: the first of full length `bs`, the second
    a single dof, every later length drawn from 1 .. bs (the last cut off at n)."""
    rng = np.random.default_rng(seed)
    blocks, first = [], 0
    while first < n:
        k = bs if not blocks else 1 if len(blocks) == 1 else int(rng.integers(1, bs + 1))
        k = min(k, n - first)
        blocks.append(list(range(first, first + k)))
        first += k
    return blocks


def strided_pairs(n):
    """Blocks {i, i + n // 2} (no runs), and the last dof on its own when n is odd: every dof covered."""
    h = n // 2
    return [[i, i + h] for i in range(h)] + ([[n - 1]] if n % 2 else [])


def uncovered_runs(n, bs, seed):
    """`ragged_runs` without about a tenth of its blocks, the last among them: their dofs are in no block."""
    blocks = ragged_runs(n, bs, seed)
    rng = np.random.default_rng(seed + 1)
    drop = set(rng.choice(np.arange(2, len(blocks) - 1), size=max(1, len(blocks) // 10 - 1), replace=False).tolist())
    drop.add(len(blocks) - 1)
    return [b for k, b in enumerate(blocks) if k not in drop]


def breakdown_dofs(n):
    """(i, i', k, k') for `exact_breakdown` with runs of 2: the first block, the blocks of lanes 255 and 256 of the
    fused kernel when there are that many (else two neighbours in the middle), the last block."""
    last = n - 1
    mid = 510 if n > 514 else 2 * ((n // 2) // 2)
    return 0, mid + 1, mid + 2, last


def exact_breakdown(n, dofs=None):
    """(A, start, blocks) with A = 2 I plus a coupling of 1 between the dofs (i, i') and (k, k'), start = 2 e_i + 2 e_k
    and blocks = runs of 2 (the four dofs in four different blocks, so that every inverse block is 0.5 I).  Every
    operation of the loop is exact: gamma_0 = 2, hist = [1, 0.5, 1, 0], rh_2 = 0, breakdown at step 1."""
    i, i2, k, k2 = breakdown_dofs(n) if dofs is None else dofs
    assert len({i // 2, i2 // 2, k // 2, k2 // 2}) == 4 and max(i, i2, k, k2) < n
    A = sp.lil_matrix((n, n))
    A.setdiag(2.0)
    for a, b in ((i, i2), (k, k2)):
        A[a, b] = A[b, a] = 1.0
    start = np.zeros(n)
    start[i] = start[k] = 2.0
    return A.tocsr(), start, [list(range(f, min(f + 2, n))) for f in range(0, n, 2)]


# ---- the cases both test files run ----------------------------------------------------------------------------------
STEPS = 8
SIZES = [1, 2, 63, 64, 65, 257, 1025]
LARGE = 2049                     # for bs >= 4: more than one workgroup of the fused kernel at every block size
FUSED_BS = [2, 3, 4, 5, 6, 7, 8]
FALLBACKS = ["bs1", "bs16", "strided", "uncovered"]


def forms_at(n):
    """The preconditioner forms run at size n.  At n <= 2 no cover can be ragged, strided or leave a dof out: point
    Jacobi, one block (bs 2) and single dofs (bs 1) remain."""
    if n <= 2:
        return ["point", "runs2", "bs1"]
    if n == LARGE:
        return ["runs%d" % bs for bs in FUSED_BS if bs >= 4] + ["bs16"]
    return ["point"] + ["runs%d" % bs for bs in FUSED_BS] + FALLBACKS


CASES = [(n, form) for n in SIZES + [LARGE] for form in forms_at(n)]


def blocks_of(n, form):
    """The cover of `form` at size n (None: point Jacobi)."""
    if form == "point":
        return None
    if form.startswith("runs"):
        return ragged_runs(n, int(form[4:]), seed=300 + n)
    return {"bs1": lambda: ragged_runs(n, 1, 0), "bs16": lambda: ragged_runs(n, 16, seed=300 + n),
            "strided": lambda: strided_pairs(n), "uncovered": lambda: uncovered_runs(n, 3, seed=300 + n)}[form]()


@functools.lru_cache(maxsize=None)
def operator(n):
    """(A as scipy CSR, A dense, the start vector) of size n (shared; read only)."""
    A = spd(n, seed=100 + n)
    start = np.random.default_rng(200 + n).standard_normal(n)
    return A, A.toarray(), start


@functools.lru_cache(maxsize=None)
def preconditioner(n, form):
    dense = operator(n)[1]
    blocks = blocks_of(n, form)
    return point_jacobi(dense) if blocks is None else BlockInverse(dense, blocks)


@functools.lru_cache(maxsize=None)
def reference(n, form):
    """The long-double recurrence of the case (shared between the tests; read only)."""
    _, dense, start = operator(n)
    return recurrence(dense, preconditioner(n, form), start, min(STEPS, n))


def worst(got, ref, count=None):
    """max |got - ref| / |delta_0| over the first `count` entries of the two histories (flattened: delta_0, gamma_1,
    delta_1, ...), in long double."""
    g, r = np.asarray(got, dtype=LD).ravel(), np.asarray(ref.hist, dtype=LD).ravel()
    count = min(g.size, r.size) if count is None else count
    return float(abs(g[:count] - r[:count]).max() / abs(r[0]))


def comparable(ref):
    """Number of history entries of `ref` that a second run can be compared on: all of them, or, with a breakdown at step
    j, the steps before it and delta_j (gamma_{j+1} is rounding noise in either run)."""
    return 2 * len(ref.hist) if ref.breakdown is None else 2 * ref.breakdown + 1
