"""Long-double statement of what the AMG V(1,1) cycle of csrc/amg.hip and the auxiliary-space term around it must compute,
for ANY list of level operators (no hierarchy set-up, no engine, nothing from oracle/), with a componentwise magnitude
bound and a derived tolerance -- shared by the joint-cycle tests.

A hierarchy here is plain host data: `levels` is the list of the non-coarsest levels, finest first, each a dict with
`A`, `P`, `R` as scipy CSR matrices and `dinv` as an array; `inv` is the coarsest-level solve as a scipy CSR matrix.

    level l:  x  = w dinv b               (pre-smoothing from 0)
              r  = b - A x
              x' = V_{l+1}(R r)           (coarsest: x' = inv b')
              x += P x'
              y  = x + w dinv (b - A x)   (post-smoothing)

Every comparison against these references is componentwise: |got_i - ref_i| <= tolerance(...) * E_i, where E is the
same computation with every operand replaced by its absolute value and every subtraction by an addition (`*_bound`)."""

import numpy as np
import scipy.sparse as sp

LD = np.longdouble
U64 = 2.0 ** -53                  # unit roundoff of fp64


def spmv_ld(mat, x):
    """mat @ x in long double, row sums in CSR order (numpy only: empty rows give 0)."""
    mat = mat.tocsr()
    prod = mat.data.astype(LD) * np.asarray(x, dtype=LD)[mat.indices]
    out = np.zeros(mat.shape[0], dtype=LD)
    live = np.flatnonzero(np.diff(mat.indptr) > 0)
    if live.size:
        out[live] = np.add.reduceat(prod, mat.indptr[live])
    return out


def _cycle(levels, inv, omega, b, l, sub):
    """`sub`: -1 for the cycle, +1 for its bound (operands already absolute)"""
    if l == len(levels):
        return spmv_ld(inv, b)
    lv = levels[l]
    wd = LD(omega) * np.asarray(lv["dinv"], dtype=LD)
    x = wd * b
    r = b + sub * spmv_ld(lv["A"], x)
    x = x + spmv_ld(lv["P"], _cycle(levels, inv, omega, spmv_ld(lv["R"], r), l + 1, sub))
    return x + wd * (b + sub * spmv_ld(lv["A"], x))


def _aux(T, TT, K, levels, inv, omega, bscale, b, sub):
    n0 = levels[0]["A"].shape[0] if levels else inv.shape[0]
    if T.shape[1] != K * n0:
        raise ValueError("T has %d columns for %d components of %d nodes" % (T.shape[1], K, n0))
    r = spmv_ld(TT, LD(bscale) * np.asarray(b, dtype=LD))
    z = np.concatenate([_cycle(levels, inv, omega, r[k * n0:(k + 1) * n0], 0, sub) for k in range(K)])
    return spmv_ld(T, z)


def cycle_ld(levels, inv, omega, b):
    return _cycle(levels, inv, omega, np.asarray(b, dtype=LD), 0, -1)


def aux_ld(T, K, levels, inv, omega, bscale, b, TT=None):
    """T (blockdiag_K cycle) T^T (bscale b) on the stacked [component][node] layout; `TT`: the transpose as it is
    applied (given when it was rounded on its own), default T^T"""
    return _aux(T, T.T.tocsr() if TT is None else TT, K, levels, inv, omega, bscale, b, -1)


def _abs(mat):
    out = sp.csr_matrix(mat, copy=True)
    out.data = np.abs(out.data)
    return out


def _abs_levels(levels):
    return [dict(A=_abs(lv["A"]), P=_abs(lv["P"]), R=_abs(lv["R"]), dinv=np.abs(lv["dinv"])) for lv in levels]


def cycle_bound(levels, inv, omega, b):
    return _cycle(_abs_levels(levels), _abs(inv), abs(omega), np.abs(np.asarray(b, dtype=LD)), 0, +1)


def aux_bound(T, K, levels, inv, omega, bscale, b, TT=None):
    TT = T.T.tocsr() if TT is None else TT
    return _aux(_abs(T), _abs(TT), K, _abs_levels(levels), _abs(inv), abs(omega), abs(bscale), np.abs(b), +1)


def longest_row(mat):
    return int(np.diff(mat.tocsr().indptr).max()) if mat.shape[0] else 0


def tolerance(levels, inv, T=None, TT=None):
    """2 * 2^-53 * sum over the kernels of one application of (longest row of that kernel's matrix + 3): the first-order
    forward bound of fp64 row sums in any order (n - 1 additions and one product per entry, up to three more rounded
    operations in the epilogue), added up along the chain of kernels -- each kernel's error is bounded relative to the
    magnitude bound E, which only grows along the chain -- and doubled for the higher-order terms and the fma / tree-sum
    differences.  Kernels: T^T and T (with `T`); per non-coarsest level the diagonal scale (row length 1), A twice, R
    and P; the coarse inverse."""
    total = longest_row(inv) + 3
    for lv in levels:
        total += (1 + 3) + 2 * (longest_row(lv["A"]) + 3) + (longest_row(lv["R"]) + 3) + (longest_row(lv["P"]) + 3)
    if T is not None:
        total += 2 * 3 + longest_row(T) + longest_row(T.T.tocsr() if TT is None else TT)
    return 2.0 * U64 * total


def round32(mat):
    out = sp.csr_matrix(mat, copy=True)
    out.data = out.data.astype(np.float32).astype(np.float64)
    return out


def round32_levels(levels):
    """fp32 storage: A, P and R rounded to fp32 values; dinv (and the coarse inverse) stay fp64 (hipla.amg.stored_levels)"""
    return [dict(A=round32(lv["A"]), P=round32(lv["P"]), R=round32(lv["R"]), dinv=lv["dinv"]) for lv in levels]


def worst_ratio(got, ref, bound, tol):
    """max_i |got_i - ref_i| / (tol * E_i); a component whose bound is 0 must be 0 exactly (ratio inf otherwise)."""
    err = np.abs(np.asarray(got, dtype=LD) - ref)
    lim = LD(tol) * bound
    ratio = np.where(lim > 0, err / np.where(lim > 0, lim, 1), np.where(err > 0, np.inf, 0.0))
    return float(ratio.max()) if ratio.size else 0.0


def check(got, ref, bound, tol, what=""):
    got = np.asarray(got)
    assert got.shape == ref.shape and np.all(np.isfinite(got)), what
    ratio = worst_ratio(got, ref, bound, tol)
    assert ratio <= 1.0, "%s: |err_i| / (tolerance * E_i) reaches %.3g (tolerance %.3g)" % (what, ratio, tol)
    return ratio
