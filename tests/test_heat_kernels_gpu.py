"""The kernels of the heat integrator (csrc/heat.hip) one at a time through the C ABI: `nss_mgs_f64`, `nss_galerkin_f64`,
`nss_basis_combine_f64` and `nss_heat_workspace`, on basis planes with a stride larger than n whose padding must come
back untouched.

Sizes: n = 1 (only the odd tail), 63 / 64 / 65 (one wave of pairs, with and without the tail), 1000 (several
workgroups), 70 001 (more than one workgroup per XCD, odd).  References are numpy in fp64 / extended precision.
Tolerances: Gram-Schmidt entries 1e-12 of the column's largest entry and |V^T V - I| <= 1e-14 d after three passes; the
Galerkin matrices the repository's 1e-13 of sum |terms| per entry; the combination 1e-15 of
sum |terms| (d <= 8 fused multiply-adds, each rounding a partial sum once: 8 * 2^-53 = 8.9e-16).

A Gaussian basis of d > n columns has no rank d: at n = 1 only d = 1 is compared, and for d > 1 the test asserts that
`norms` reports the deficiency (which is what `heat.evolve` checks)."""

import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

import heat_reference as hr

pytestmark = pytest.mark.gpu

LD = np.longdouble
SENT = -7.25
DIMS = (1, 2, 5, 8)


class Planes:
    """A basis of d planes of stride ld > n on the device, padding filled with SENT."""

    def __init__(self, eng, columns, pad=6):
        self.eng = eng
        self.n, self.d = len(columns[0]), len(columns)
        self.ld = self.n + pad + (self.n + pad) % 2
        host = np.full(self.d * self.ld, SENT)
        for k, col in enumerate(columns):
            host[k * self.ld:k * self.ld + self.n] = col
        self.buf = eng.from_host(host)
        count = C.c_int64()
        eng._check(eng.lib.nss_heat_workspace(self.n, self.d, C.byref(count)))
        self.work = eng.zeros(count.value)

    def host(self):
        """(columns [d, n], padding intact)"""
        out = self.eng.to_host(self.buf).reshape(self.d, self.ld)
        return out[:, :self.n].copy(), bool((out[:, self.n:] == SENT).all())

    def mgs(self, tries):
        eng = self.eng
        norms = eng.from_host(np.full(tries * self.d, SENT))
        eng._check(eng.lib.nss_mgs_f64(self.n, self.d, self.ld, self.buf.data_ptr(), tries, norms.data_ptr(),
                                       self.work.data_ptr(), self.work.numel(), eng.stream))
        return eng.to_host(norms).reshape(tries, self.d)

    def galerkin(self, mat):
        eng = self.eng
        g = eng.zeros(self.d * self.d)
        rc = eng.lib.nss_galerkin_f64(mat.handle.ptr, self.d, self.ld, self.buf.data_ptr(), g.data_ptr(),
                                      self.work.data_ptr(), self.work.numel(), eng.stream)
        return rc, eng.to_host(g).reshape(self.d, self.d)


def refused(eng, rc, word):
    msg = eng.lib.nss_last_error().decode()
    assert rc != 0 and word in msg, (rc, msg)


# ---- nss_mgs_f64 ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 63, 64, 65, 1000, 70001])
def test_mgs_gaussian_bases(hip_engine, n):
    rng = np.random.default_rng(n)
    for d in DIMS:
        start = [rng.standard_normal(n) for _ in range(d)]
        for tries in (1, 3):
            planes = Planes(hip_engine, start)
            norms = planes.mgs(tries)
            got, intact = planes.host()
            assert intact, (n, d, tries)
            if d > n:                                            # no rank d: the norms must say so
                assert not (np.isfinite(norms).all() and (norms > 0).all()), (n, d, tries)
                continue
            ref = np.array(hr.numpy_mgs([c.copy() for c in start], tries))
            assert np.isfinite(norms).all() and (norms > 0).all()
            assert abs(norms[0, 0] - start[0] @ start[0]) <= 1e-14 * (start[0] @ start[0])    # |b_0|^2 of the input
            for k in range(d):
                assert np.abs(got[k] - ref[k]).max() <= 1e-12 * np.abs(ref[k]).max(), (n, d, tries, k)
            if tries == 3:
                assert np.abs(got @ got.T - np.eye(d)).max() <= 1e-14 * d, (n, d)
                again = Planes(hip_engine, start)                # the same bits on a second run
                norms2 = again.mgs(tries)
                assert np.array_equal(again.host()[0], got) and np.array_equal(norms2, norms), (n, d)


def test_mgs_ill_conditioned_krylov_basis(hip_engine):
    """The sub-step vectors of the last (fifth) step of the n = 33 run with time step 1e-2 (condition 3.5e9; the first
    step's is 8.6e6): the last column of Q moves by condition x rounding, so no entries are compared -- orthogonality and
    the nested spans are."""
    K, m, start, _ = hr.restated(33, 1e-2)
    before_last, _, steps = hr.dense_evolve(start, 0.035, 1e-2, K, m)
    assert steps == 4
    columns = hr.krylov_columns(before_last, K, m, 1e-2)
    B = np.array(columns)
    sv = np.linalg.svd(B / np.linalg.norm(B, axis=1)[:, None], compute_uv=False)
    assert sv[0] / sv[-1] > 1e9
    planes = Planes(hip_engine, columns)
    norms = planes.mgs(3)
    Q, intact = planes.host()
    d = len(columns)
    assert intact and np.isfinite(norms).all() and (norms > 0).all()
    assert np.abs(Q @ Q.T - np.eye(d)).max() <= 1e-14 * d
    for k in range(d):
        r = B[k].astype(LD)
        for _ in range(2):
            r = r - Q[:k + 1].T.astype(LD) @ (Q[:k + 1].astype(LD) @ r)
        assert float(np.sqrt(r @ r)) <= 1e-12 * np.linalg.norm(B[k]), k
    again = Planes(hip_engine, columns)
    again.mgs(3)
    assert np.array_equal(again.host()[0], Q)


# ---- nss_galerkin_f64 -----------------------------------------------------------------------------------------------
def random_rows(rng, n):
    """n x n CSR with 0 .. 9 entries per row (empty rows included), random columns, duplicates kept apart."""
    counts = rng.integers(0, 10, size=n)
    counts[rng.integers(0, n)] = 0
    if n > 1:
        counts[rng.integers(0, n)] = 9
    indptr = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    cols = rng.integers(0, n, size=int(indptr[-1])).astype(np.int32)
    mat = sp.csr_matrix((rng.standard_normal(cols.size), cols, indptr), shape=(n, n))
    mat.sort_indices()
    return mat


def galerkin_reference(mat, V):
    """(V^T (M V), |V|^T (|M| |V|)) with the row sums and the column sums in extended precision; V: [d, n]."""
    prod = mat.data.astype(LD)[:, None] * V.T[mat.indices].astype(LD)
    W = np.zeros((mat.shape[0], V.shape[0]), dtype=LD)
    has = np.diff(mat.indptr) > 0
    if prod.size:
        W[has] = np.add.reduceat(prod, mat.indptr[:-1][has], axis=0)
        absW = np.zeros_like(W)
        absW[has] = np.add.reduceat(np.abs(prod), mat.indptr[:-1][has], axis=0)
    else:
        absW = np.zeros_like(W)
    return V.astype(LD) @ W, np.asarray(np.abs(V).astype(LD) @ absW, dtype=np.float64)


@pytest.mark.parametrize("n", [1, 65, 1000, 70001])
def test_galerkin_random_matrices(hip_engine, n):
    import hipla
    rng = np.random.default_rng(100 + n)
    mats = [random_rows(rng, n)]
    assert (np.diff(mats[0].indptr) == 0).any()
    if n == 1:
        mats.append(sp.csr_matrix(np.array([[-1.5]])))             # (the random 1 x 1 matrix is its empty row)
    worst = 0.0
    for mat in mats:
        device = hipla.SparseMatrix.from_scipy(mat)
        for d in DIMS:
            V = rng.standard_normal((d, n))
            planes = Planes(hip_engine, list(V))
            rc, G = planes.galerkin(device)
            assert rc == 0, hip_engine.lib.nss_last_error()
            ref, scale = galerkin_reference(mat, V)
            err = np.abs(np.asarray(G.astype(LD) - ref, dtype=np.float64))
            ok = scale > 0
            assert (err[~ok] == 0).all()
            if ok.any():
                worst = max(worst, float((err[ok] / scale[ok]).max()))
            assert (err <= 1e-13 * scale).all(), (n, d)
            rc2, G2 = planes.galerkin(device)
            assert rc2 == 0 and np.array_equal(G, G2) and planes.host()[1]
    print("n %d: largest error %.2e of sum |terms|" % (n, worst))


def test_galerkin_refuses_fp32_values(hip_engine):
    import hipla
    mat = hipla.SparseMatrix.from_scipy(random_rows(np.random.default_rng(1), 65))
    hip_engine.csr_narrow_f32(mat.handle)
    assert hip_engine.csr_value_bytes(mat.handle) == 4 * mat.handle.nnz
    planes = Planes(hip_engine, [np.ones(65)])
    rc, G = planes.galerkin(mat)
    refused(hip_engine, rc, "fp32")
    assert (G == 0).all()


# ---- nss_basis_combine_f64 ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 63, 64, 65, 1000, 70001])
def test_basis_combine(hip_engine, n):
    eng = hip_engine
    rng = np.random.default_rng(200 + n)
    for d in DIMS:
        V = rng.standard_normal((d, n))
        coeff = rng.standard_normal(d)
        ref = coeff.astype(LD) @ V.astype(LD)
        scale = np.abs(coeff) @ np.abs(V)
        for alias in (False, True):
            planes = Planes(eng, list(V))
            y = planes.buf[:n] if alias else eng.from_host(np.full(n + 2, SENT))
            harr = (C.c_double * d)(*coeff)
            eng._check(eng.lib.nss_basis_combine_f64(n, d, planes.ld, planes.buf.data_ptr(), harr, y.data_ptr(),
                                                     eng.stream))
            got = eng.to_host(y)
            if not alias:
                assert (got[n:] == SENT).all()
            err = np.abs(np.asarray(got[:n].astype(LD) - ref, dtype=np.float64))
            assert (err <= 1e-15 * scale).all(), (n, d, alias)
            after, intact = planes.host()
            assert intact and np.array_equal(after[1:], V[1:])
            assert np.array_equal(after[0], got[:n] if alias else V[0])


# ---- refusals ---------------------------------------------------------------------------------------------------------
def test_refusals_launch_nothing(hip_engine):
    import hipla
    eng, lib = hip_engine, hip_engine.lib
    n = 65
    planes = Planes(eng, [np.ones(n), np.arange(n, dtype=np.float64)])
    before = eng.to_host(planes.buf).copy()
    norms, g = eng.from_host(np.full(8, SENT)), eng.from_host(np.full(64, SENT))
    square = hipla.SparseMatrix.from_scipy(sp.identity(n, format="csr"))
    wide = hipla.SparseMatrix.from_scipy(sp.csr_matrix(np.ones((n, n + 1))))
    b, w, cap, st = planes.buf.data_ptr(), planes.work.data_ptr(), planes.work.numel(), eng.stream
    coeff = (C.c_double * 8)(*([1.0] * 8))
    y = eng.from_host(np.full(n, SENT))
    count = C.c_int64(-1)
    for d in (0, 9):
        refused(eng, lib.nss_mgs_f64(n, d, planes.ld, b, 3, norms.data_ptr(), w, cap, st), "mgs")
        refused(eng, lib.nss_galerkin_f64(square.handle.ptr, d, planes.ld, b, g.data_ptr(), w, cap, st), "galerkin")
        refused(eng, lib.nss_basis_combine_f64(n, d, planes.ld, b, coeff, y.data_ptr(), st), "basis_combine")
        refused(eng, lib.nss_heat_workspace(n, d, C.byref(count)), "heat_workspace")
    refused(eng, lib.nss_mgs_f64(n, 2, planes.ld, None, 3, norms.data_ptr(), w, cap, st), "NULL")
    refused(eng, lib.nss_mgs_f64(n, 2, planes.ld, b, 3, None, w, cap, st), "NULL")
    refused(eng, lib.nss_mgs_f64(n, 2, planes.ld, b, 3, norms.data_ptr(), None, cap, st), "NULL")
    refused(eng, lib.nss_mgs_f64(n, 2, planes.ld, b, 3, norms.data_ptr(), w, 8, st), "work")
    refused(eng, lib.nss_mgs_f64(n, 2, n - 1, b, 3, norms.data_ptr(), w, cap, st), "stride")
    refused(eng, lib.nss_galerkin_f64(None, 2, planes.ld, b, g.data_ptr(), w, cap, st), "NULL")
    refused(eng, lib.nss_galerkin_f64(square.handle.ptr, 2, planes.ld, None, g.data_ptr(), w, cap, st), "NULL")
    refused(eng, lib.nss_galerkin_f64(square.handle.ptr, 2, planes.ld, b, None, w, cap, st), "NULL")
    refused(eng, lib.nss_galerkin_f64(wide.handle.ptr, 2, planes.ld, b, g.data_ptr(), w, cap, st), "square")
    refused(eng, lib.nss_basis_combine_f64(n, 2, planes.ld, None, coeff, y.data_ptr(), st), "NULL")
    refused(eng, lib.nss_basis_combine_f64(n, 2, planes.ld, b, None, y.data_ptr(), st), "NULL")
    refused(eng, lib.nss_basis_combine_f64(n, 2, planes.ld, b, coeff, None, st), "NULL")
    assert count.value == -1
    assert np.array_equal(eng.to_host(planes.buf), before)
    assert (eng.to_host(norms) == SENT).all() and (eng.to_host(g) == SENT).all() and (eng.to_host(y) == SENT).all()
