"""Fast diagonalisation (Lynch, Rice & Thomas 1964) of an operator that is a Kronecker sum over the axes of a
tensor-product grid,

    Lp = T_0 (x) I (x) I  +  I (x) T_1 (x) I  +  I (x) I (x) T_2,        T_a = Q_a diag(lambda_a) Q_a^T,

    Lp^-1 rhs = (Q_0 (x) Q_1 (x) Q_2) [ 1 / (lambda_0[i] + lambda_1[j] + lambda_2[k]) ] (Q_0^T (x) Q_1^T (x) Q_2^T) rhs:

2 d dense contractions along one grid axis each, no iteration, no tolerance.  The pressure operator B M_u^-1 B^T of every
system of this package is of that form.  `fdm_factors` finds the factors on the host and checks
them against the matrix entry by entry; `FastDiagonalization` applies the inverse -- ``nss_fdm_solve_f64`` on the HIP
engine (csrc/fdm.hip), the numpy restatement of the same formula on any other.

The velocity operator and the scalar's diffusion operator have the same structure per component of their vector:
`component_factors` finds the factors of every component and checks the layout the kernel addresses, and
`ComponentFastDiagonalization` applies ``(diag(mass) + sigma mat)^-1`` for any sigma with one set of factors --
``nss_fdmc_solve_f64`` (csrc/fdm_components.hip) or the numpy restatement.

Without a mass the same factors give the inverse of the velocity operator itself: `inverse_factors` runs the checks of
`component_factors` and asks that the operator be definite, and `FastDiagonalizationInverse` applies ``mat^-1`` as a
preconditioner of the Stokes solvers -- ``nss_fdmi_apply_f64`` (csrc/fdm_inverse.hip), inside the
fused loops on the HIP engine, or the numpy restatement.

`gather_factors` reads the same 1-D factors off a matrix that is resident on the HIP engine (``nss_fdm_gather_factors``,
csrc/fdm_gather.hip) without fetching it; the proof that the matrix is their Kronecker sum is the
host's."""

import ctypes as C
import os

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


def gather_available(eng):
    """Whether `eng` is the HIP engine with the entry point that reads the factors off a resident matrix."""
    return _hip(eng) and hasattr(getattr(eng, "lib", None), "nss_fdm_gather_factors")


def gather_factors(mat, bases, pitch, shapes):
    """The 1-D factors of the resident `mat` (a `SparseMatrix` of the HIP engine) on components laid out as
    `component_factors` asks -- entry (k, j, i) of component c at ``bases[c] + k * pitch + j * e_2 + i``, `shapes` their
    extents -- by the rule of `fdm_factors`, without fetching the matrix: T_a[x, y] = mat[line_a[x], line_a[y]] on the
    grid line through the component's origin is gathered on the device (``nss_fdm_gather_factors``; DESIGN.md section
    19), e x e doubles per axis are downloaded, and (d - 1) / d * mat[origin, origin] is taken off the diagonal here, the
    same fp64 operation on the same operands as on the host: for a matrix without duplicates the arrays EQUAL the
    ``FdmFactors.T`` of the host.  Per component the list of its d arrays.  Nothing is proved about the rest of the
    matrix.  ``ValueError`` when the engine or the matrix cannot do it (not the HIP engine, not a `SparseMatrix`, fp32
    storage, a layout the library refuses)."""
    from .hip_engine import NssError
    if not isinstance(mat, SparseMatrix):
        raise ValueError("gather_factors: the matrix is a %s, not a SparseMatrix" % type(mat).__name__)
    eng = mat.engine
    if not gather_available(eng):
        raise ValueError("gather_factors: the engine %r has no nss_fdm_gather_factors" % (getattr(eng, "name", eng),))
    shapes = [tuple(int(e) for e in s) for s in shapes]
    ncomp, d = len(shapes), len(shapes[0]) if shapes else 0
    if not 1 <= ncomp <= 3 or d not in (2, 3) or any(len(s) != d or min(s) < 1 for s in shapes) or len(bases) != ncomp:
        raise ValueError("gather_factors: one to three components over two, or over three, positive extents each, and "
                         "a base for each")
    base = (C.c_int64 * ncomp)(*[int(b) for b in bases])
    ext = (C.c_int64 * (ncomp * d))(*[e for s in shapes for e in s])
    T = [[np.zeros((e, e)) for e in s] for s in shapes]
    out = (C.c_void_p * (ncomp * d))(*[t.ctypes.data for ts in T for t in ts])
    try:
        eng._check(eng.lib.nss_fdm_gather_factors(mat.handle.ptr, ncomp, d, mat.m, base, int(pitch), ext, out,
                                                  eng.stream))
    except NssError as err:
        raise ValueError("gather_factors: %s" % err)
    for ts in T:
        corner = ts[0][0, 0]
        for t in ts:
            t[np.diag_indices(t.shape[0])] -= (d - 1) / d * corner
    return T


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


# ---- the shifted solve on the components of an interleaved vector ------------------------------
class ComponentFactors:
    """What `component_factors` returns: `n_total`; `pitch` (the distance of two slabs, one for all components); per
    component `bases`, `extents`, `ids` (the flat id arrays), `factors` (its `FdmFactors`) and `masses` (its uniform
    lumped mass)."""

    def __init__(self, n_total, pitch, bases, ids, factors, masses):
        self.n_total, self.pitch, self.bases = int(n_total), int(pitch), [int(b) for b in bases]
        self.ids, self.factors, self.masses = ids, factors, [float(m) for m in masses]
        self.extents = [f.extents for f in factors]

    @property
    def dim(self):
        return self.factors[0].dim

    def solve(self, rhs, sigma):
        """The numpy restatement of ``(diag(mass) + sigma mat)^-1 rhs``: per component Q_a^T along every axis, the
        scaling by 1 / (m + sigma sums()), Q_a along every axis."""
        rhs = np.asarray(rhs, dtype=np.float64)
        out = rhs.copy()
        for ids, f, m in zip(self.ids, self.factors, self.masses):
            w = rhs[ids].reshape(f.extents)
            for a, q in enumerate(f.Q):
                w = np.moveaxis(np.tensordot(q.T, w, axes=(1, a)), 0, a)
            w = w * (1.0 / (m + sigma * f.sums()))
            for a, q in enumerate(f.Q):
                w = np.moveaxis(np.tensordot(q, w, axes=(1, a)), 0, a)
            out[ids] = np.ascontiguousarray(w).reshape(-1)
        return out


def _affine_layout(components, n_total):
    """(bases, pitch) of id arrays whose entry (k, j, i) is base + k * pitch + j * e_2 + i, or the reason why not."""
    bases, pitches, slabs = [], set(), []
    dims = {g.ndim for g in components}
    if len(dims) != 1 or not dims <= {2, 3}:
        return "the components are not all arrays over two, or all over three, axes"
    for c, g in enumerate(components):
        if g.size == 0 or g.min() < 0 or g.max() >= n_total:
            return "component %d is empty or holds ids outside 0 .. %d" % (c, n_total - 1)
        slab = int(np.prod(g.shape[1:], dtype=np.int64))
        base = int(g.flat[0])
        pitch = int(g[(1,) + (0,) * (g.ndim - 1)]) - base if g.shape[0] > 1 else slab
        want = base + np.arange(g.shape[0], dtype=np.int64).reshape((-1,) + (1,) * (g.ndim - 1)) * pitch \
            + np.arange(slab, dtype=np.int64).reshape(g.shape[1:])
        if not np.array_equal(g, want):
            return "the ids of component %d are not affine: base + k * pitch + j * e_2 + i" % c
        if g.shape[0] > 1:
            if pitch < slab:
                return "the slabs of component %d overlap (pitch %d, %d entries per slab)" % (c, pitch, slab)
            pitches.add(pitch)
        bases.append(base)
        slabs.append(slab)
    if len(pitches) > 1:
        return "the components have different pitches: %s" % sorted(pitches)
    return bases, (pitches.pop() if pitches else max(slabs))


def component_factors(mat, components, mass):
    """The factors of ``diag(mass) + sigma mat`` for the direct solve on components: (`ComponentFactors`, None), or
    (None, reason) -- nothing is raised.  `mat`: scipy sparse, square; `components`: integer id arrays shaped by their
    grid extents (`StokesSystem.component_ids`, or ``[np.arange(n_p).reshape((n,) * dim)]`` for a cell-centred scalar);
    `mass`: the lumped mass, one value or one per row.  Declined unless the ids are affine in (base, pitch) with one pitch,
    the components are disjoint and cover every row, no entry of `mat` couples two components, every component's
    sub-matrix passes `fdm_factors` over its extents, the mass is constant and positive on each component, and no sum of
    eigenvalues is below -TOLERANCE max |sum| (the operator is positive semi-definite on it)."""
    if mass is None:
        return None, "no mass (the pure inverse: inverse_factors)"
    try:
        return _component_factors(mat, components, mass)
    except Exception as err:                                # the promise of the docstring: a reason, never a raise
        return None, "%s: %s" % (type(err).__name__, err)


def inverse_factors(mat, components):
    """The factors of ``mat^-1`` on components: (`ComponentFactors` with the masses 0, None), or (None, reason) -- nothing
    is raised.  The checks of `component_factors` without a mass (layout, coverage, no coupling, `fdm_factors` per
    component); declined as well when a sum of eigenvalues is not above TOLERANCE max |sum|: `mat` must be definite.  The
    velocity operator of an enclosed cavity is; a singular operator has no inverse to offer."""
    try:
        return _component_factors(mat, components, None)
    except Exception as err:                                # the promise of the docstring: a reason, never a raise
        return None, "%s: %s" % (type(err).__name__, err)


def _component_factors(mat, components, mass):
    """`mass` None: the factors of the pure inverse (`inverse_factors`)."""
    import scipy.sparse as sp
    if not sp.issparse(mat) or mat.shape[0] != mat.shape[1]:
        return None, "the matrix is not sparse and square"
    n_total = mat.shape[0]
    if n_total > 2 ** 31 - 1:
        return None, "more than 2^31 - 1 rows"
    components = [np.asarray(g) for g in components]
    if not 1 <= len(components) <= 3 or not all(np.issubdtype(g.dtype, np.integer) for g in components):
        return None, "the components are not one to three integer id arrays"
    components = [g.astype(np.int64) for g in components]
    layout = _affine_layout(components, n_total)
    if isinstance(layout, str):
        return None, layout
    bases, pitch = layout
    flat = [np.ascontiguousarray(g.reshape(-1)) for g in components]
    label = np.full(n_total, -1, dtype=np.int64)
    for c, ids in enumerate(flat):
        if (label[ids] >= 0).any():
            return None, "component %d overlaps an earlier one" % c
        label[ids] = c
    if (label < 0).any():
        return None, "the components miss %d of the %d rows (the first: row %d)" \
            % (int((label < 0).sum()), n_total, int(np.flatnonzero(label < 0)[0]))
    coo = sp.coo_matrix(mat)
    coupling = (label[coo.row] != label[coo.col]) & (coo.data != 0)
    if coupling.any():
        at = int(np.flatnonzero(coupling)[0])
        return None, "the entry (%d, %d) couples the components %d and %d" \
            % (coo.row[at], coo.col[at], label[coo.row[at]], label[coo.col[at]])
    pure = mass is None
    m = np.zeros(n_total) if pure else np.asarray(mass, dtype=np.float64)
    m = np.full(n_total, float(m)) if m.ndim == 0 else m
    if m.shape != (n_total,):
        return None, "the mass holds %s entries for %d rows" % (m.shape, n_total)
    csr = sp.csr_matrix(mat)
    factors, masses = [], []
    for c, (g, ids) in enumerate(zip(components, flat)):
        mc = m[ids]
        if not pure and not (np.isfinite(mc).all() and (mc == mc[0]).all() and mc[0] > 0.0):
            return None, "the mass is not constant and positive on component %d" % c
        made, why = fdm_factors(csr[ids][:, ids], g.shape)
        if made is None:
            return None, "component %d: %s" % (c, why)
        sums = made.sums()
        if pure and not sums.min() > TOLERANCE * abs(sums).max():
            return None, "component %d has the eigenvalue sum %.3g, not above %g max |sum|: the operator is not definite " \
                "and has no inverse" % (c, sums.min(), TOLERANCE)
        if sums.min() < -TOLERANCE * abs(sums).max():
            return None, "component %d has the eigenvalue sum %.3g, below -%g max |sum|" % (c, sums.min(), TOLERANCE)
        factors.append(made)
        masses.append(mc[0])
    return ComponentFactors(n_total, pitch, bases, flat, factors, masses), None


class _FdmcHandle(_FdmHandle):
    def __del__(self):
        try:
            if self.ptr:
                self.engine.lib.nss_fdmc_destroy(self.ptr)
                self.ptr = None
        except Exception:
            pass


def create_component_handle(eng, cf):
    """The ``nss_fdmc_t`` of the `ComponentFactors` `cf` on the HIP engine `eng`."""
    ncomp, d = len(cf.factors), cf.dim
    base = (C.c_int64 * ncomp)(*cf.bases)
    ext = (C.c_int64 * (ncomp * d))(*[e for f in cf.factors for e in f.extents])
    qs = (C.c_void_p * (ncomp * d))(*[q.ctypes.data for f in cf.factors for q in f.Q])
    lams = (C.c_void_p * (ncomp * d))(*[w.ctypes.data for f in cf.factors for w in f.lam])
    mass = (C.c_double * ncomp)(*cf.masses)
    out = C.c_void_p()
    eng._check(eng.lib.nss_fdmc_create(ncomp, d, cf.n_total, base, cf.pitch, ext, qs, lams, mass, C.byref(out)))
    return _FdmcHandle(eng, out)


def components_available(eng):
    """Whether `eng` is the HIP engine with the component entry points."""
    return _hip(eng) and hasattr(getattr(eng, "lib", None), "nss_fdmc_solve_f64")


class ComponentFastDiagonalization(BaseMatrix, FusedLoop):
    """``y = (diag(mass) + sigma mat)^-1 x`` by fast diagonalisation on the components of the vector, for a `mat` that
    `component_factors` accepts (``ValueError`` with the reason otherwise; `try_create` returns None instead, the reason in
    ``ComponentFastDiagonalization.last_declined``).  `mat`: a `SparseMatrix` or scipy sparse.  `sigma` is a property: the
    factors do not depend on it, so one object serves every step size.  On the HIP engine `Mult` is
    ``nss_fdmc_solve_f64`` (2 dim launches for all components, no host synchronisation); on any other engine the numpy
    restatement of the same formula.

    A direct solve: `iterations` is 0, and `precision` / `maxsteps` are there to be set and are ignored, so that the
    object can stand where a `CGSolver` stands."""

    iterations = 0

    @classmethod
    def try_create(cls, mat, components, mass, sigma, engine=None):
        factors, why = component_factors(mat.to_scipy() if isinstance(mat, SparseMatrix) else mat, components, mass)
        return cls._decided(why if factors is None else cls(mat, components, mass, sigma, engine, factors))

    def __init__(self, mat, components, mass, sigma, engine=None, factors=None):
        super().__init__()
        if factors is None:
            factors, why = component_factors(mat.to_scipy() if isinstance(mat, SparseMatrix) else mat, components, mass)
            if factors is None:
                raise ValueError("ComponentFastDiagonalization: " + why)
        if engine is None:
            from .engine import get_engine
            engine = mat.engine if isinstance(mat, SparseMatrix) else get_engine()
        self.engine, self.factors = engine, factors
        self.n = factors.n_total
        self.sigma = sigma
        self.precision, self.maxsteps, self.errors = None, None, []
        self.handle = create_component_handle(engine, factors) if components_available(engine) else None

    @property
    def sigma(self):
        return self._sigma

    @sigma.setter
    def sigma(self, value):
        value = float(value)
        if not (value >= 0.0 and np.isfinite(value)):
            raise ValueError("ComponentFastDiagonalization: sigma is non-negative and finite, not %r" % (value,))
        self._sigma = value

    def Height(self):
        return self.n

    def Width(self):
        return self.n

    def solve_resident(self, rhs, out, sigma=None):
        """out = (diag(mass) + sigma mat)^-1 rhs on device buffers of the HIP engine (distinct ones); `sigma` None: the
        object's.  Returns the iterations: 0."""
        eng = self.engine
        eng._check(eng.lib.nss_fdmc_solve_f64(self.handle.ptr, self._sigma if sigma is None else float(sigma),
                                              rhs.data_ptr(), out.data_ptr(), eng.stream))
        return 0

    def Mult(self, x, y):
        if len(x) != self.n or len(y) != self.n:
            raise ValueError("ComponentFastDiagonalization: the operator is %d x %d, x holds %d and y %d entries"
                             % (self.n, self.n, len(x), len(y)))
        if self.handle is not None and isinstance(x, Vector) and isinstance(y, Vector):
            src = x.Copy() if self.engine.overlaps(x.buf, y.buf) else x
            self.solve_resident(src.buf, y.buf)
            return
        y.data = Vector.from_numpy(self.factors.solve(x.numpy(), self._sigma), engine=y.engine)

    MultTrans = Mult          # symmetric

    @property
    def T(self):
        return self


# ---- the pure inverse as a preconditioner of the Stokes solvers ---------------------------------
class _FdmiHandle(_FdmHandle):
    def __del__(self):
        try:
            if self.ptr:
                self.engine.lib.nss_fdmi_destroy(self.ptr)
                self.ptr = None
        except Exception:
            pass


def create_inverse_handle(eng, cf):
    """The ``nss_fdmi_t`` of the `ComponentFactors` `cf` (of `inverse_factors`) on the HIP engine `eng`."""
    ncomp, d = len(cf.factors), cf.dim
    base = (C.c_int64 * ncomp)(*cf.bases)
    ext = (C.c_int64 * (ncomp * d))(*[e for f in cf.factors for e in f.extents])
    qs = (C.c_void_p * (ncomp * d))(*[q.ctypes.data for f in cf.factors for q in f.Q])
    lams = (C.c_void_p * (ncomp * d))(*[w.ctypes.data for f in cf.factors for w in f.lam])
    out = C.c_void_p()
    eng._check(eng.lib.nss_fdmi_create(ncomp, d, cf.n_total, base, cf.pitch, ext, qs, lams, C.byref(out)))
    return _FdmiHandle(eng, out)


def inverse_available(eng):
    """Whether `eng` is the HIP engine with the entry points of the inverse."""
    return _hip(eng) and hasattr(getattr(eng, "lib", None), "nss_fdmi_apply_f64")


class FastDiagonalizationInverse(BaseMatrix, FusedLoop):
    """``y = mat^-1 x`` by fast diagonalisation on the components of the vector, for a `mat` that `inverse_factors` accepts
    (``ValueError`` with the reason otherwise; `try_create` returns None instead, the reason in
    ``FastDiagonalizationInverse.last_declined``).  `mat`: a `SparseMatrix` or scipy sparse; `components`: the id arrays
    (`StokesSystem.component_ids`).  Symmetric: ``.T`` is the object itself.

    The exact inverse of the velocity block as ``preA`` of `BramblePasciakCG`, `bramble_pasciak_cg` and `MinRes`: on the
    HIP engine the fused loops apply it themselves (``nss_fdmi_apply_f64``: 2 dim launches for all components, a scale in
    the epilogue, no host synchronisation), and `Mult` is the same call; on any other engine `Mult` is the numpy
    restatement, ``ComponentFactors.solve(x, 1.0)`` with the masses 0.

    `tile` picks the tile body of the native contractions (``nss_fdmi_set_tile``): -1 the library's choice, 0 the FMA tile
    of csrc/fdm_tile.h, 1 the matrix-core tile of csrc/fdm_tile_mfma.h.  It is a property of the object, not of the
    process; a new object starts from the environment variable ``NSS_FDM_TILE`` (unset or empty: -1)."""

    @classmethod
    def try_create(cls, mat, components, engine=None):
        factors, why = inverse_factors(mat.to_scipy() if isinstance(mat, SparseMatrix) else mat, components)
        return cls._decided(why if factors is None else cls(mat, components, engine, factors))

    def __init__(self, mat, components, engine=None, factors=None):
        super().__init__()
        if factors is None:
            factors, why = inverse_factors(mat.to_scipy() if isinstance(mat, SparseMatrix) else mat, components)
            if factors is None:
                raise ValueError("FastDiagonalizationInverse: " + why)
        if engine is None:
            from .engine import get_engine
            engine = mat.engine if isinstance(mat, SparseMatrix) else get_engine()
        self.engine, self.factors = engine, factors
        self.n = factors.n_total
        self.handle = create_inverse_handle(engine, factors) if inverse_available(engine) else None
        self._tile = -1
        self.tile = int(os.environ.get("NSS_FDM_TILE") or -1)

    @property
    def tile(self):
        return self._tile

    @tile.setter
    def tile(self, mode):
        mode = int(mode)
        if mode not in (-1, 0, 1):
            raise ValueError("FastDiagonalizationInverse: the tile is -1 (the library's choice), 0 (FMA) or 1 (matrix "
                             "cores), not %r" % (mode,))
        if self.handle is not None:
            self.engine._check(self.engine.lib.nss_fdmi_set_tile(self.handle.ptr, mode))
        self._tile = mode

    def Height(self):
        return self.n

    def Width(self):
        return self.n

    def apply_resident(self, x, y, scale=1.0):
        """y = scale mat^-1 x on device buffers of the HIP engine (distinct ones)."""
        eng = self.engine
        eng._check(eng.lib.nss_fdmi_apply_f64(self.handle.ptr, float(scale), x.data_ptr(), y.data_ptr(), None, eng.stream))

    def Mult(self, x, y):
        if len(x) != self.n or len(y) != self.n:
            raise ValueError("FastDiagonalizationInverse: the operator is %d x %d, x holds %d and y %d entries"
                             % (self.n, self.n, len(x), len(y)))
        if self.handle is not None and isinstance(x, Vector) and isinstance(y, Vector):
            src = x.Copy() if self.engine.overlaps(x.buf, y.buf) else x
            self.apply_resident(src.buf, y.buf)
            return
        y.data = Vector.from_numpy(self.factors.solve(x.numpy(), 1.0), engine=y.engine)

    MultTrans = Mult          # symmetric

    @property
    def T(self):
        return self
