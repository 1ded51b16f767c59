"""Saddle-point systems [[A, B^T], [B, 0]] no grid produces, at the sizes where the element-wise kernels of the three
fused saddle-point loops branch (csrc/bpcg2.hip: bpcg2_k4_kernel; csrc/minres.hip: minres_m3_kernel, minres_m4_kernel:
two elements per lane, 512 per workgroup, a scalar tail for the last element of an odd part, the velocity and the pressure
part in workgroup ranges of their own).  Host only: numpy and scipy, no engine.

`SIZES` puts each part one below, at and one above 512 and 1024, one part inside a single wave, n_p = 1 beside a long
velocity part, and both parities of each part.  tests/test_saddle_cases_cpu.py shows that the oracle alone meets the
conditions the GPU tests (tests/test_saddle_loop_edges_gpu.py) rest on."""

import functools

import numpy as np
import scipy.linalg as sla
import scipy.sparse as sp

SIZES = [(1, 1), (2, 1), (3, 2), (63, 1), (65, 64), (511, 255), (512, 512), (513, 511), (1023, 513), (1025, 1),
         (1537, 1025)]


def seed_of(n_u, n_p):
    return 1000 * n_u + n_p


def system(n_u, n_p, seed):
    """(A, B, f, g, mass).  A = diag(d) + 0.5 S / |S|_inf with d in [1, 2) and S = R + R^T, R with 0 to 3 random
    entries per row and none in the rows i % 7 == 3 (S empty: A is the diagonal): sorted CSR, SPD by diagonal dominance,
    the eigenvalues of D^-1 A within about [0.78, 1.22].  B = a random n_p x n_u matrix of density min(1, 3 / n_u) plus a
    private entry in [2, 3) at column r (n_u // n_p) of row r: full row rank, B^T with empty rows at most sizes.  mass in
    [0.5, 1.5); f, g standard normal."""
    rng = np.random.default_rng(seed)
    d = 1.0 + rng.random(n_u)
    rows, cols, vals = [], [], []
    for i in range(n_u):
        count = 0 if i % 7 == 3 else int(rng.integers(0, 4))
        for j in rng.integers(0, n_u, size=count):
            rows.append(i)
            cols.append(int(j))
            vals.append(rng.standard_normal())
    R = sp.csr_matrix((vals, (rows, cols)), shape=(n_u, n_u))
    S = (R + R.T).tocsr()
    norm = abs(S).sum(axis=1).max() if S.nnz else 0.0
    A = sp.diags(d).tocsr()
    if norm > 0.0:
        A = (A + (0.5 / norm) * S).tocsr()
    A.sum_duplicates()
    A.sort_indices()
    B = sp.random(n_p, n_u, density=min(1.0, 3.0 / n_u), random_state=np.random.RandomState(seed % (2 ** 31)),
                  data_rvs=rng.standard_normal).tolil()
    for r in range(n_p):
        B[r, r * (n_u // n_p)] = 2.0 + rng.random()
    B = B.tocsr()
    B.sort_indices()
    mass = 0.5 + rng.random(n_p)
    f, g = rng.standard_normal(n_u), rng.standard_normal(n_p)
    return A, B, f, g, mass


@functools.lru_cache(maxsize=None)
def case(n_u, n_p):
    """`system` at the seed of the size (shared between the tests: leave the operands unchanged)."""
    return system(n_u, n_p, seed_of(n_u, n_p))


def dense_of(pre, n):
    """The matrix of the callable `pre` (x -> P x)."""
    return np.column_stack([pre(e) for e in np.eye(n)])


def scale(A, pre):
    """k = 1 / lambda_min(pre A) + 1e-3: the formula of `krylov_ref.scale_factor` with the exact minimum, from a dense
    symmetric eigen-solve (the eigenvalues of P A are those of L^T P L, A = L L^T).  A preconditioner that maps some
    dofs to zero (block Jacobi with dofs in no block) is singular; every iterate of the three methods then stays zero at
    those dofs and the run is the run on the system without them: the minimum is taken over that system."""
    n = A.shape[0]
    P = dense_of(pre, n)
    keep = np.abs(P).sum(axis=1) > 0.0
    L = np.linalg.cholesky(A.toarray()[np.ix_(keep, keep)])
    lam = sla.eigvalsh(L.T @ P[np.ix_(keep, keep)] @ L)
    return 1.0 / float(lam[0]) + 1e-3


def runs(n_u, lengths):
    """Blocks of consecutive dofs whose lengths cycle through `lengths`, the last cut short at n_u (list of lists)."""
    out, first, k = [], 0, 0
    while first < n_u:
        last = min(n_u, first + lengths[k % len(lengths)])
        out.append(list(range(first, last)))
        first, k = last, k + 1
    return out


def table(blocks):
    """(bs, nblocks) index table with -1 padding, as `krylov_ref.block_jacobi` takes it."""
    idx = -np.ones((max(len(b) for b in blocks), len(blocks)), dtype=np.int64)
    for k, b in enumerate(blocks):
        idx[: len(b), k] = b
    return idx


def dense_solution(A, B, f, g, keep=None):
    """[u; p] of [[A, B^T], [B, 0]] [u; p] = [f; g] by a dense solve.  `keep` (boolean, n_u): the velocity dofs a
    singular preconditioner leaves free; the others are held at zero (their rows and columns are dropped)."""
    n_u, n_p = A.shape[0], B.shape[0]
    keep = np.ones(n_u, dtype=bool) if keep is None else np.asarray(keep, dtype=bool)
    Ad, Bd = A.toarray()[np.ix_(keep, keep)], B.toarray()[:, keep]
    K = np.block([[Ad, Bd.T], [Bd, np.zeros((n_p, n_p))]])
    x = np.linalg.solve(K, np.concatenate([f[keep], g]))
    u = np.zeros(n_u)
    u[keep] = x[: int(keep.sum())]
    return np.concatenate([u, x[int(keep.sum()):]])


def permuted(A, B, f, g, mass, seed):
    """The symmetrically permuted twin (A[pi][:, pi], B[sigma][:, pi], f[pi], g[sigma], mass[sigma]) and (pi, sigma):
    the same problem with different rounding."""
    rng = np.random.default_rng(seed)
    pi, sigma = rng.permutation(A.shape[0]), rng.permutation(B.shape[0])
    Ap = A[pi][:, pi].tocsr()
    Bp = B[sigma][:, pi].tocsr()
    Ap.sort_indices()
    Bp.sort_indices()
    return (Ap, Bp, f[pi], g[sigma], mass[sigma]), (pi, sigma)


METHODS = ("bpcg2", "bpcg1", "minres")


def reference(method, ops, pa, ps, k, tol, maxsteps):
    """(iterations done, [u; p], history) of the oracle restatement of `method` (oracle/krylov_ref.py) on
    ops = (A, B, f, g).  The history is what the method's entry point records: sqrt(|<w, d>|) per iteration for
    BPCG v2, err_i / err_0 for the textbook BPCG and MINRES (first entry 1)."""
    from oracle import krylov_ref as kr
    A, B, f, g = ops
    with np.errstate(all="ignore"):
        if method == "bpcg2":
            it, u, p, hist = kr.bpcg_v2(A, B, pa, ps, f, g, k, tol=tol, maxsteps=maxsteps)[:4]
            return it + 1, np.concatenate([u, p]), np.array(hist)
        if method == "bpcg1":
            u, p, errors, converged = kr.bpcg_v1(A, B, pa, ps, f, g, k, tolerance=tol, max_steps=maxsteps)
            return len(errors) - (1 if converged else 0), np.concatenate([u, p]), np.array(errors)
        u, p, errors, _ = kr.minres(A, B, pa, ps, f, g, maxsteps=maxsteps, tol=tol)
        return len(errors) - 1, np.concatenate([u, p]), np.array(errors)


def distance(x, ref):
    """|x - ref| / |ref| (|x| when the reference is zero)."""
    norm = np.linalg.norm(ref)
    return np.linalg.norm(x - ref) / (norm if norm > 0.0 else 1.0)
