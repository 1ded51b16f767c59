"""Fast diagonalisation (Lynch, Rice & Thomas 1964) of an operator that is a Kronecker sum over the axes of a
tensor-product grid,

    Lp = T_0 (x) I (x) I  +  I (x) T_1 (x) I  +  I (x) I (x) T_2,        T_a = Q_a diag(lambda_a) Q_a^T,

    Lp^-1 rhs = (Q_0 (x) Q_1 (x) Q_2) [ 1 / (lambda_0[i] + lambda_1[j] + lambda_2[k]) ] (Q_0^T (x) Q_1^T (x) Q_2^T) rhs:

2 d dense contractions along one grid axis each, no iteration, no tolerance.  The pressure operator B M_u^-1 B^T of every
system of this package is of that form.  `fdm_factors` finds the factors on the host and checks
them against the matrix entry by entry; `FastDiagonalization` applies the inverse -- ``nss_fdm_solve_f64`` on the HIP
engine (csrc/fdm.hip), the numpy restatement of the same formula on any other."""

import ctypes as C

import numpy as np

from .fused import FusedLoop, _hip
from .matrix import BaseMatrix, SparseMatrix
from .vector import Vector

TOLERANCE = 1e-12           # of the entry-by-entry comparison, relative to max |Lp|, and of the null threshold


class FdmFactors:
    """What `fdm_factors` returns: `extents`; per axis `T` (the 1-D factor), `Q` (its eigenvectors, in columns) and `lam`
    (its eigenvalues); `null_threshold`: a mode whose |lambda_0[i] + lambda_1[j] + ...| is not above it is zeroed (its
    multiplier is 0); `error` = max |Lp - K| / max |Lp| of the comparison."""

    def __init__(self, extents, T, error):
        self.extents, self.T, self.error = tuple(extents), T, error
        eig = [np.linalg.eigh(t) for t in T]
        self.lam = [np.ascontiguousarray(w, dtype=np.float64) for w, _ in eig]
        self.Q = [np.ascontiguousarray(q, dtype=np.float64) for _, q in eig]
        sums = self.sums()
        self.null_threshold = TOLERANCE * float(abs(sums).max())
        self.zeroed = int((abs(sums) <= self.null_threshold).sum())

    @property
    def dim(self):
        return len(self.extents)

    def sums(self):
        """lambda_0[i] + lambda_1[j] (+ lambda_2[k]) on the grid, added in that order."""
        d = self.dim
        out = self.lam[0].reshape((-1,) + (1,) * (d - 1))
        for a in range(1, d):
            out = out + self.lam[a].reshape((1,) * a + (-1,) + (1,) * (d - 1 - a))
        return out

    def multipliers(self):
        """1 / sums(), 0 at the zeroed modes."""
        sums = self.sums()
        null = abs(sums) <= self.null_threshold
        return np.where(null, 0.0, 1.0 / np.where(null, 1.0, sums))

    def kronecker_sum(self):
        return kronecker_sum(self.T)

    def solve(self, rhs):
        """The numpy restatement of the solve: the component of `rhs` along the zeroed modes is dropped, and the
        result has none -- for the enclosed cavity (one zeroed mode, the constants) it has mean zero."""
        w = np.asarray(rhs, dtype=np.float64).reshape(self.extents)
        for a, q in enumerate(self.Q):                       # Q_a^T along every axis
            w = np.moveaxis(np.tensordot(q.T, w, axes=(1, a)), 0, a)
        w = w * self.multipliers()
        for a, q in enumerate(self.Q):                       # Q_a along every axis
            w = np.moveaxis(np.tensordot(q, w, axes=(1, a)), 0, a)
        return np.ascontiguousarray(w).reshape(-1)


def kronecker_sum(T):
    """sum_a I (x) T_a (x) I as a scipy CSR matrix with sorted indices and no stored zeros."""
    import scipy.sparse as sp
    sizes = [t.shape[0] for t in T]
    total = None
    for a, t in enumerate(T):
        term = sp.kron(sp.kron(sp.identity(int(np.prod(sizes[:a], dtype=np.int64))), sp.csr_matrix(t)),
                       sp.identity(int(np.prod(sizes[a + 1:], dtype=np.int64))), format="csr")
        total = term if total is None else total + term
    total = total.tocsr()
    total.eliminate_zeros()
    total.sort_indices()
    return total


def fdm_factors(Lp, extents):
    """The factors of `Lp` (scipy CSR, cells in lexicographic order over `extents`, last axis fastest) as a Kronecker sum:
    (`FdmFactors`, None), or (None, reason) when `Lp` is not one -- nothing is raised.

    For axis a, T_a takes its off-diagonal entries from the rows and columns of the grid line through the origin along a,
    and its diagonal is Lp[p, p] - (d - 1) / d * Lp[0, 0] at the points p of that line: one valid split of the diagonal,
    since only the sum over the axes enters.  The Kronecker sum K of the factors is then compared with `Lp` entry by
    entry; the factors are declined when the patterns differ or max |Lp - K| > 1e-12 max |Lp|."""
    import scipy.sparse as sp
    try:
        extents = tuple(int(e) for e in extents)
    except (TypeError, ValueError):
        return None, "the extents are not integers"
    d = len(extents)
    if d not in (2, 3) or min(extents) < 1:
        return None, "the extents %r are not two or three positive numbers" % (extents,)
    cells = int(np.prod(extents, dtype=np.int64))
    if cells > 2 ** 31 - 1:
        return None, "more than 2^31 - 1 cells"
    if not sp.issparse(Lp) or Lp.shape != (cells, cells):
        return None, "the matrix is not sparse and %d x %d (the extents %r)" % (cells, cells, extents)
    L = sp.csr_matrix(Lp, dtype=np.float64, copy=True)
    L.sum_duplicates()
    L.eliminate_zeros()
    L.sort_indices()
    top = float(abs(L.data).max()) if L.nnz else 0.0
    if not top > 0.0 or not np.isfinite(L.data).all():
        return None, "the matrix is zero or not finite"
    corner = L[0, 0]
    T = []
    for a, e in enumerate(extents):
        line = np.arange(e, dtype=np.int64) * int(np.prod(extents[a + 1:], dtype=np.int64))
        t = L[line][:, line].toarray()
        t[np.diag_indices(e)] -= (d - 1) / d * corner
        T.append(t)
    K = kronecker_sum(T)
    diff = abs(L - K)
    error = (float(diff.max()) if diff.nnz else 0.0) / top
    if error > TOLERANCE:
        return None, "max |Lp - K| = %.3g max |Lp| (more than %g): not a Kronecker sum over these extents" \
            % (error, TOLERANCE)
    if not (np.array_equal(L.indptr, K.indptr) and np.array_equal(L.indices, K.indices)):
        return None, "the pattern is not that of a Kronecker sum over these extents"
    return FdmFactors(extents, T, error), None


class _FdmHandle:
    def __init__(self, engine, ptr):
        self.engine, self.ptr = engine, ptr

    def __del__(self):
        try:
            if self.ptr:
                self.engine.lib.nss_fdm_destroy(self.ptr)
                self.ptr = None
        except Exception:
            pass


def create_handle(eng, factors):
    """The ``nss_fdm_t`` of `factors` on the HIP engine `eng`: the d matrices and eigenvalue vectors uploaded, and the two
    work buffers of prod(extents) doubles a solve ping-pongs between."""
    d = factors.dim
    ext = (C.c_int64 * d)(*factors.extents)
    qs = (C.c_void_p * d)(*[q.ctypes.data for q in factors.Q])
    lams = (C.c_void_p * d)(*[w.ctypes.data for w in factors.lam])
    out = C.c_void_p()
    eng._check(eng.lib.nss_fdm_create(d, ext, qs, lams, factors.null_threshold, C.byref(out)))
    return _FdmHandle(eng, out)


def available(eng):
    """Whether `eng` is the HIP engine with the fast-diagonalisation entry points."""
    return _hip(eng) and hasattr(getattr(eng, "lib", None), "nss_fdm_solve_f64")


class FastDiagonalization(BaseMatrix, FusedLoop):
    """``y = Lp^-1 x`` by fast diagonalisation, for an `Lp` that `fdm_factors` accepts over `extents` (``ValueError`` with
    the reason otherwise; `try_create` returns None instead, the reason in ``FastDiagonalization.last_declined``).  `Lp`:
    a `SparseMatrix` or a scipy CSR matrix.  On the HIP engine `Mult` is ``nss_fdm_solve_f64`` (2 d launches, no host
    synchronisation); on any other engine it runs the numpy restatement of the same formula over ``.numpy()``.

    A direct solve: `iterations` is 0, and `precision` / `maxsteps` are there to be set and are ignored, so that the object
    can stand where a `CGSolver` stands.  A singular `Lp` (the enclosed cavity: the constants) has its null modes zeroed:
    the result then has no component along them -- mean zero -- and differs from a CG solve's by a constant, which no
    gradient sees."""

    iterations = 0

    @classmethod
    def try_create(cls, Lp, extents, engine=None):
        mat = Lp.to_scipy() if isinstance(Lp, SparseMatrix) else Lp
        factors, why = fdm_factors(mat, extents)
        return cls._decided(why if factors is None else cls(Lp, extents, engine, factors))

    def __init__(self, Lp, extents, engine=None, factors=None):
        super().__init__()
        if factors is None:
            factors, why = fdm_factors(Lp.to_scipy() if isinstance(Lp, SparseMatrix) else Lp, extents)
            if factors is None:
                raise ValueError("FastDiagonalization: " + why)
        if engine is None:
            from .engine import get_engine
            engine = Lp.engine if isinstance(Lp, SparseMatrix) else get_engine()
        self.engine, self.factors = engine, factors
        self.n = int(np.prod(factors.extents, dtype=np.int64))
        self.precision, self.maxsteps, self.errors = None, None, []
        self.handle = create_handle(engine, factors) if available(engine) else None

    def Height(self):
        return self.n

    def Width(self):
        return self.n

    def solve_resident(self, rhs, phi):
        """phi = Lp^-1 rhs on device buffers of the HIP engine (distinct ones); returns the iterations: 0."""
        eng = self.engine
        eng._check(eng.lib.nss_fdm_solve_f64(self.handle.ptr, rhs.data_ptr(), phi.data_ptr(), eng.stream))
        return 0

    def Mult(self, x, y):
        if len(x) != self.n or len(y) != self.n:
            raise ValueError("FastDiagonalization: the operator is %d x %d, x holds %d and y %d entries"
                             % (self.n, self.n, len(x), len(y)))
        if self.handle is not None and isinstance(x, Vector) and isinstance(y, Vector):
            src = x.Copy() if self.engine.overlaps(x.buf, y.buf) else x
            self.solve_resident(src.buf, y.buf)
            return
        y.data = Vector.from_numpy(self.factors.solve(x.numpy()), engine=y.engine)

    MultTrans = Mult          # Lp symmetric

    @property
    def T(self):
        return self
