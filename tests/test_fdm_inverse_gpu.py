"""The inverse of the velocity block by fast diagonalisation on the product engine (csrc/fdm_inverse.hip, DESIGN.md
section 18): the lane maps of the matrix-core tile on exact integer data, the rounding of both tiles against long double,
the apply on the operators of the grid, the loop contract (`done`, untouched entries, refusals), and the three Stokes
solvers with the new preconditioner inside their fused loops against the oracle driven by a sparse LU of A.

Bounds, with u = 2^-53.  One contraction sums n products; whatever the order of the sum -- one FMA per term, or four
terms per matrix instruction -- it errs by at most gamma_n (|M| |x|) per output, and 2 (n + 2) u (|M| |x|) covers the
products of the (1 + gamma) of a chain: the bound of tests/test_fdm_gpu.py, valid for both tiles without measurement.
An apply is 2 dim such passes and the scaling by scale / sum (two additions, a division, a product: 4 u), so per entry

    |y - exact| <= c u |scale| (|Q_0| (x) ..) |1 / sum| (|Q_0^T| (x) ..) |x|,

with c = the sum over the 2 dim passes of 2 (n_a + 2), + 6."""

import contextlib
import ctypes as C
import io

import numpy as np
import pytest
import scipy.sparse.linalg as spl

from conftest import iteration_tolerance

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
LD = np.longdouble
SENT = -7.25                       # what output buffers hold before a launch
GUARD = 96                         # doubles in front of and behind an output
EXTENTS = [(1, 1), (3, 5), (4, 64), (15, 17), (16, 16), (17, 130), (65, 66), (130, 3)]      # (n, nq)
TILES = {"fma": 0, "mfma": 1}
# The history of a loop against the oracle's.  A~ A f - f cancels three digits (k - 1 = 1e-3), so the history feels the
# rounding of preA: measured on the CPU, the oracle driven by a sparse LU and by ComponentFactors.solve differ by at most
# 3.3e-7 (relative, entry by entry, all three solvers, the four cases of LOOP_CASES; the largest: 3-D n = 17, BPCG v1).
HISTORY_MEASURED = 3.3e-7
HISTORY_TOL = 10 * HISTORY_MEASURED
LOOP_CASES = [(2, 12), (2, 18), (3, 6), (3, 17)]


def guarded_output(eng, count):
    whole = eng.from_host(np.full(count + 2 * GUARD, SENT))
    return whole, eng.view(whole, GUARD, GUARD + count)


def contract(eng, M, X, transpose, lines, tile, done=None):
    """nss_fdmi_contract_f64 with the tile `tile` on host arrays; X is (n, nq) for lines = 0 and (nq, n) for lines = 1."""
    n = M.shape[0]
    nq = X.shape[0] if lines else X.shape[1]
    dM, dX = eng.from_host(np.ascontiguousarray(M).ravel()), eng.from_host(np.ascontiguousarray(X).ravel())
    whole, out = guarded_output(eng, n * nq)
    rc = eng.lib.nss_fdmi_contract_f64(n, nq, lines, tile, dM.data_ptr(), transpose, dX.data_ptr(), out.data_ptr(),
                                       None if done is None else done.data_ptr(), eng.stream)
    assert rc == 0, eng.lib.nss_last_error()
    got = eng.to_host(whole)
    assert (got[:GUARD] == SENT).all() and (got[GUARD + n * nq:] == SENT).all()
    return got[GUARD: GUARD + n * nq].reshape(X.shape)


def product(M, X, transpose, lines):
    Mop = M.T if transpose else M
    return X @ Mop.T if lines else Mop @ X


@pytest.mark.parametrize("n,nq", EXTENTS)
def test_lane_maps_on_exact_integer_data(hip_engine, n, nq):
    """Integer entries of magnitude <= 8: every product and every partial sum is an integer below 2^53, so each order of
    summation gives the same bits and the result must EQUAL numpy's integer product.  M is not symmetric, and X has no
    structure: a row or column of the accumulator stored in the wrong place cannot pass."""
    eng = hip_engine
    rng = np.random.default_rng(100 * n + nq)
    M = rng.integers(-8, 9, size=(n, n))
    for lines in (0, 1):
        X = rng.integers(-8, 9, size=(nq, n) if lines else (n, nq))
        for transpose in (0, 1):
            want = product(M, X, transpose, lines).astype(np.float64)
            for name, mode in TILES.items():
                got = contract(eng, M.astype(np.float64), X.astype(np.float64), transpose, lines, mode)
                assert np.array_equal(got, want), (name, lines, transpose)


@pytest.mark.parametrize("n,nq", EXTENTS)
def test_rounding_of_both_tiles_against_long_double(hip_engine, n, nq):
    eng = hip_engine
    rng = np.random.default_rng(200 * n + nq)
    M = rng.standard_normal((n, n))
    for lines in (0, 1):
        X = rng.standard_normal((nq, n) if lines else (n, nq))
        for transpose in (0, 1):
            want = product(M.astype(LD), X.astype(LD), transpose, lines)
            bound = 2 * (n + 2) * U * product(np.abs(M), np.abs(X), transpose, lines)
            for name, mode in TILES.items():
                got = contract(eng, M, X, transpose, lines, mode)
                err = np.abs(got.astype(LD) - want).astype(np.float64)
                assert (err <= bound).all(), (name, lines, transpose, float((err / bound).max()))


def test_the_two_tiles_are_deterministic_and_differ_by_rounding_at_most(hip_engine):
    eng = hip_engine
    rng = np.random.default_rng(3)
    M, X = rng.standard_normal((65, 65)), rng.standard_normal((65, 66))
    out = {}
    for name, mode in TILES.items():
        out[name] = contract(eng, M, X, 0, 0, mode)
        assert np.array_equal(contract(eng, M, X, 0, 0, mode), out[name])    # the same bits every run
    assert np.allclose(out["fma"], out["mfma"], rtol=0.0, atol=4 * 67 * U * (np.abs(M) @ np.abs(X)).max())
    # (on the MI355X the two have been seen to agree in every bit -- profiles/fdm_stokes.md -- which nothing promises)


# ---- the apply --------------------------------------------------------------------------------------------------------
def along(M, w, a):
    return np.moveaxis(np.tensordot(M, w, axes=(1, a)), 0, a)


def long_double_solve(cf, x, scale):
    """`ComponentFactors.solve(x, 1.0)` with the masses 0, times `scale`, in long double."""
    out = x.astype(LD)
    for ids, f in zip(cf.ids, cf.factors):
        w = x[ids].reshape(f.extents).astype(LD)
        for a, q in enumerate(f.Q):
            w = along(q.T.astype(LD), w, a)
        sums = f.lam[0].astype(LD).reshape((-1,) + (1,) * (f.dim - 1))
        for a in range(1, f.dim):
            sums = sums + f.lam[a].astype(LD).reshape((1,) * a + (-1,) + (1,) * (f.dim - 1 - a))
        w = w * (LD(scale) / sums)
        for a, q in enumerate(f.Q):
            w = along(q.astype(LD), w, a)
        out[ids] = w.reshape(-1)
    return out


@pytest.mark.parametrize("dim,n", [(2, 5), (2, 18), (2, 66), (3, 4), (3, 17)])
def test_apply_on_the_grid_operators(hip_engine, dim, n):
    import hipla
    from staggered_grid import mac_stokes
    eng = hip_engine
    s = mac_stokes(dim, n, 0.01)
    A = hipla.SparseMatrix.from_scipy(s.A)
    pre = hipla.FastDiagonalizationInverse(A, s.component_ids)
    assert pre.handle is not None
    x = np.random.default_rng(7).standard_normal(s.n_u)
    dx = eng.from_host(x)
    for scale in (1.0, 1.001):
        exact = long_double_solve(pre.factors, x, scale)
        host = scale * pre.factors.solve(x, 1.0)
        host_err = float(np.linalg.norm((host.astype(LD) - exact).astype(np.float64)))
        assert host_err > 0.0
        for name, mode in TILES.items():
            whole, out = guarded_output(eng, s.n_u)
            pre.tile = mode
            pre.apply_resident(dx, out, scale)
            got = eng.to_host(whole)
            assert (got[:GUARD] == SENT).all() and (got[GUARD + s.n_u:] == SENT).all()
            y = got[GUARD: GUARD + s.n_u]
            err = float(np.linalg.norm((y.astype(LD) - exact).astype(np.float64)))
            print("apply %d-D n = %d scale %g tile %s: error / error of the numpy restatement = %.3f"
                  % (dim, n, scale, name, err / host_err))
            assert err <= 8.0 * host_err, (name, scale, err / host_err)
    # Mult is the same call
    pre.tile = -1
    with pytest.raises(ValueError, match="tile"):
        pre.tile = 2
    assert pre.tile == -1
    vx, vy = hipla.Vector.from_numpy(x), hipla.Vector(s.n_u)
    vy.data = pre * vx
    whole, out = guarded_output(eng, s.n_u)
    pre.apply_resident(dx, out, 1.0)
    assert np.array_equal(vy.numpy(), eng.to_host(out))


def synthetic(extents, base, pitch, tail, seed=0):
    rng = np.random.default_rng(seed)
    slab = int(np.prod(extents[1:]))
    n_total = base + (extents[0] - 1) * pitch + slab + tail
    Q = [np.ascontiguousarray(rng.standard_normal((e, e))) for e in extents]
    lam = [np.ascontiguousarray(0.5 + rng.random(e)) for e in extents]
    k = np.arange(extents[0]).reshape((-1,) + (1,) * (len(extents) - 1))
    ids = base + k * pitch + np.arange(slab).reshape(extents[1:])
    return n_total, Q, lam, ids


class Handle:
    def __init__(self, eng, n_total, extents, base, pitch, Q, lam):
        d = len(extents)
        self.keep = (Q, lam)
        out = C.c_void_p()
        rc = eng.lib.nss_fdmi_create(1, d, n_total, (C.c_int64 * 1)(base), pitch, (C.c_int64 * d)(*extents),
                                     (C.c_void_p * d)(*[q.ctypes.data for q in Q]),
                                     (C.c_void_p * d)(*[w.ctypes.data for w in lam]), C.byref(out))
        assert rc == 0 and out.value, eng.lib.nss_last_error()
        self.eng, self.ptr = eng, out

    def __del__(self):
        if self.ptr:
            self.eng.lib.nss_fdmi_destroy(self.ptr)
            self.ptr = None


@pytest.mark.parametrize("extents,base,pitch,tail", [((3, 4, 5), 3, 29, 4), ((2, 66, 3), 1, 199, 2), ((65, 4), 1, 5, 2),
                                                     ((4, 65), 1, 66, 2)])
def test_loop_contract_on_a_padded_scalar_layout(hip_engine, extents, base, pitch, tail):
    """One component in a padded buffer: NaNs around the component in x, sentinels in y.  The component's entries obey the
    bound of the module docstring, every other entry of y keeps its bits, `done` = 1 leaves all of y alone."""
    eng = hip_engine
    n_total, Q, lam, ids = synthetic(extents, base, pitch, tail)
    h = Handle(eng, n_total, extents, base, pitch, Q, lam)
    rng = np.random.default_rng(11)
    x = np.full(n_total, np.nan)
    x[ids.ravel()] = rng.standard_normal(ids.size)
    d = len(extents)
    sums = lam[0].reshape((-1,) + (1,) * (d - 1))
    for a in range(1, d):
        sums = sums + lam[a].reshape((1,) * a + (-1,) + (1,) * (d - 1 - a))
    scale = 1.001
    want, chain = x[ids].astype(LD), np.abs(x[ids])
    for a, q in enumerate(Q):
        want, chain = along(q.T.astype(LD), want, a), along(np.abs(q.T), chain, a)
    want, chain = want * (LD(scale) / sums.astype(LD)), chain * (scale / sums)
    for a, q in enumerate(Q):
        want, chain = along(q.astype(LD), want, a), along(np.abs(q), chain, a)
    c = sum(2 * 2 * (e + 2) for e in extents) + 6
    dx = eng.from_host(x)
    one = eng.torch.ones(1, dtype=eng.torch.int32, device=eng.device)
    zero = eng.torch.zeros(1, dtype=eng.torch.int32, device=eng.device)
    for name, mode in TILES.items():
        assert eng.lib.nss_fdmi_set_tile(h.ptr, mode) == 0
        whole, out = guarded_output(eng, n_total)
        assert eng.lib.nss_fdmi_apply_f64(h.ptr, scale, dx.data_ptr(), out.data_ptr(), one.data_ptr(), eng.stream) == 0
        assert (eng.to_host(whole) == SENT).all(), name                          # done: nothing is written
        assert eng.lib.nss_fdmi_apply_f64(h.ptr, scale, dx.data_ptr(), out.data_ptr(), zero.data_ptr(), eng.stream) == 0
        got = eng.to_host(whole)
        y = got[GUARD: GUARD + n_total]
        outside = np.ones(n_total, dtype=bool)
        outside[ids.ravel()] = False
        assert (got[:GUARD] == SENT).all() and (got[GUARD + n_total:] == SENT).all() and (y[outside] == SENT).all(), name
        err = np.abs(y[ids].astype(LD) - want).astype(np.float64)
        assert np.isfinite(y[ids]).all() and (err <= c * U * chain).all(), (name, float((err / (c * U * chain)).max()))


def test_argument_errors_are_codes_not_faults(hip_engine):
    eng, lib = hip_engine, hip_engine.lib
    extents, base, pitch, tail = (3, 4, 5), 3, 29, 4
    n_total, Q, lam, _ = synthetic(extents, base, pitch, tail)
    h = Handle(eng, n_total, extents, base, pitch, Q, lam)
    x, y = eng.zeros(n_total), eng.zeros(n_total)
    ok = lambda: b"fdmi" in lib.nss_last_error()
    assert lib.nss_fdmi_apply_f64(h.ptr, 1.0, x.data_ptr(), x.data_ptr(), None, eng.stream) != 0 and ok()     # aliasing
    assert lib.nss_fdmi_apply_f64(h.ptr, 1.0, None, y.data_ptr(), None, eng.stream) != 0 and ok()
    assert lib.nss_fdmi_apply_f64(h.ptr, 1.0, x.data_ptr(), None, None, eng.stream) != 0 and ok()
    assert lib.nss_fdmi_apply_f64(None, 1.0, x.data_ptr(), y.data_ptr(), None, eng.stream) != 0 and ok()
    assert lib.nss_fdmi_apply_f64(h.ptr, float("nan"), x.data_ptr(), y.data_ptr(), None, eng.stream) != 0 and ok()
    m = eng.zeros(16)
    mp, xp, yp = m.data_ptr(), x.data_ptr(), y.data_ptr()
    assert lib.nss_fdmi_contract_f64(4, 4, 0, -1, mp, 0, xp, xp, None, eng.stream) != 0 and ok()              # aliasing
    assert lib.nss_fdmi_contract_f64(4, 4, 0, -1, None, 0, xp, yp, None, eng.stream) != 0 and ok()
    assert lib.nss_fdmi_contract_f64(0, 4, 0, -1, mp, 0, xp, yp, None, eng.stream) != 0 and ok()
    assert lib.nss_fdmi_contract_f64(4, 4, 0, 2, mp, 0, xp, yp, None, eng.stream) != 0 and ok()               # no such tile
    assert lib.nss_fdmi_contract_f64(2 ** 20, 2 ** 20, 0, -1, mp, 0, xp, yp, None, eng.stream) != 0
    assert lib.nss_fdmi_set_tile(h.ptr, 2) != 0 and ok() and lib.nss_fdmi_set_tile(h.ptr, -2) != 0
    assert lib.nss_fdmi_set_tile(None, 0) != 0 and ok()
    out = C.c_void_p()
    d = len(extents)
    args = dict(ncomp=1, dim=d, n_total=n_total, base=(C.c_int64 * 1)(base), pitch=pitch, ext=(C.c_int64 * d)(*extents),
                q=(C.c_void_p * d)(*[q.ctypes.data for q in Q]), lam=(C.c_void_p * d)(*[w.ctypes.data for w in lam]))

    def create(**change):
        a = dict(args, **change)
        return lib.nss_fdmi_create(a["ncomp"], a["dim"], a["n_total"], a["base"], a["pitch"], a["ext"], a["q"], a["lam"],
                                   a.get("out", C.byref(out)))
    singular = [np.ascontiguousarray(w - w.min()) for w in lam]             # the least sum of eigenvalues is 0
    bad = [dict(ncomp=0), dict(dim=4), dict(n_total=0), dict(pitch=0), dict(pitch=19), dict(base=(C.c_int64 * 1)(-1)),
           dict(n_total=n_total - tail - 1), dict(ext=(C.c_int64 * d)(3, 0, 5)), dict(q=None), dict(out=None),
           dict(lam=(C.c_void_p * d)(*[w.ctypes.data for w in singular])),
           dict(lam=(C.c_void_p * d)(lam[0].ctypes.data, None, lam[2].ctypes.data))]
    for change in bad:
        assert create(**change) != 0, list(change)
        assert b"fdmi_create" in lib.nss_last_error() and not out.value, (list(change), lib.nss_last_error())


# ---- the fused loops --------------------------------------------------------------------------------------------------
class Form:
    def __init__(self, mat):
        self.mat, self.condense = mat, False


_ORACLE = {}


def oracle(dim, n):
    """The three oracle runs of a case with a sparse LU of A as pre_a, computed once."""
    if (dim, n) not in _ORACLE:
        from oracle import krylov_ref as kr
        from staggered_grid import mac_stokes
        s = mac_stokes(dim, n, 0.01)
        f, g = s.rhs(0)
        lu = spl.splu(s.A.tocsc())
        pm = kr.diag_inverse(s.mass)
        k = kr.scale_factor(kr.lanczos_ritz(s.A, lu.solve, tol=1e-3))
        it2, u2, p2, h2, _ = kr.bpcg_v2(s.A, s.B, lu.solve, pm, f, g, k, tol=1e-8, maxsteps=500)
        u1, p1, e1, _ = kr.bpcg_v1(s.A, s.B, lu.solve, pm, f, g, k, tolerance=1e-8, max_steps=500)
        um, pmr, em, _ = kr.minres(s.A, s.B, lu.solve, pm, f, g, maxsteps=500, tol=1e-8)
        _ORACLE[(dim, n)] = dict(s=s, f=f, g=g, k=k, v2=(u2, p2, np.asarray(h2)), v1=(u1, p1, np.asarray(e1)),
                                 minres=(um, pmr, np.asarray(em)))
    return _ORACLE[(dim, n)]


def residuals(s, f, g, u, p):
    return np.linalg.norm(s.A @ u + s.B.T @ p - f) / np.linalg.norm(f), np.linalg.norm(s.B @ u - g)


def check_against(o, which, u, p, hist):
    s, f, g = o["s"], o["f"], o["g"]
    u_ref, p_ref, h_ref = o[which]
    assert abs(len(hist) - len(h_ref)) <= iteration_tolerance({"iterations": len(h_ref)}), (which, len(hist), len(h_ref))
    m = min(len(hist), len(h_ref))
    rel = np.abs(np.asarray(hist[:m]) - h_ref[:m]) / np.abs(h_ref[:m])
    print("%s: %d iterations (oracle %d), history within %.3g" % (which, len(hist) - 1, len(h_ref) - 1, rel.max()))
    assert rel.max() <= HISTORY_TOL, (which, float(rel.max()))
    r_ref, d_ref = residuals(s, f, g, u_ref, p_ref)
    r, d = residuals(s, f, g, u, p)
    print("%s: residual %.3g (oracle %.3g), divergence %.3g (oracle %.3g)" % (which, r, r_ref, d, d_ref))
    assert r <= 10 * r_ref and d <= 10 * d_ref, (which, r, r_ref, d, d_ref)


@pytest.mark.parametrize("tile_name", list(TILES))
@pytest.mark.parametrize("dim,n", LOOP_CASES)
def test_solvers_run_fused_with_the_inverse(hip_engine, dim, n, tile_name):
    import hipla
    from bramble_pasciak_cg import bramble_pasciak_cg
    from hipla import fused
    from minres import MinRes
    from solvers.bramblepasciak_new import BpcgSession
    eng = hip_engine
    o = oracle(dim, n)
    s, f, g = o["s"], o["f"], o["g"]
    with contextlib.redirect_stdout(io.StringIO()) as quiet:
        A, B = hipla.SparseMatrix.from_scipy(s.A), hipla.SparseMatrix.from_scipy(s.B)
        pre = hipla.FastDiagonalizationInverse(A, s.component_ids)
        pre.tile = TILES[tile_name]
        preM = hipla.DiagonalMatrix(1.0 / s.mass)
        fv, gv = hipla.Vector.from_numpy(f), hipla.Vector.from_numpy(g)
        # the scale factor: pre * A = I, the native Lanczos breaks down after one step with the Ritz value 1
        info = {}
        ritz = hipla.la.EigenValues_Preconditioner(mat=A, pre=pre, tol=1e-3, info=info)
        # BPCG v2
        sol = hipla.BlockVector([hipla.Vector(s.n_u), hipla.Vector(s.n_p)])
        ses = BpcgSession(Form(A), Form(B), None, fv, gv, pre, preM, sol=sol)
        declined2 = ses.fused_declined
        ses.first_direction()
        it2, hist2, conv2 = ses.fused.run(ses.wdn, ses.err0, 1e-8, True, 500)
        # BPCG v1
        sol1, errs1 = bramble_pasciak_cg(A, B, None, pre, preM, fv, gv, tolerance=1e-8, max_steps=500, print_rates=False)
        declined1 = fused.Bpcg1Loop.last_declined
        # MINRES
        K = hipla.BlockMatrix([[A, B.T], [B, None]])
        Cm = hipla.BlockMatrix([[pre, None], [None, preM]])
        um, errsm = MinRes(mat=K, pre=Cm, rhs=hipla.BlockVector([fv, gv]), maxsteps=500, tol=1e-8, printrates=False)
        declinedm = fused.MinresLoop.last_declined
    assert info["native"] and len(ritz) >= 1 and np.all(np.isfinite(ritz))
    assert abs(ritz.min() - 1.0) <= 1e-9 and abs(ritz.max() - 1.0) <= 1e-9, ritz
    assert abs(ses.k - 1.001) <= 1e-8 and ses.lanczos_native
    assert declined2 is None and declined1 is None and declinedm is None, (declined2, declined1, declinedm)
    assert conv2 and "Warning" not in quiet.getvalue()
    check_against(o, "v2", sol[0].numpy(), sol[1].numpy(), np.asarray(hist2))
    check_against(o, "v1", sol1[0].numpy(), sol1[1].numpy(), np.asarray(errs1))
    check_against(o, "minres", um[0].numpy(), um[1].numpy(), np.asarray(errsm))


def test_minres_takes_a_scaled_inverse(hip_engine):
    """MINRES carries no k: the scale of a scaled inverse goes into the loop state (pre_fdm_scale) and from there into
    the epilogue of the apply.  Against the oracle with 2.5 times the sparse LU solve."""
    import hipla
    from hipla import fused
    from minres import MinRes
    from oracle import krylov_ref as kr
    o = oracle(2, 12)
    s, f, g = o["s"], o["f"], o["g"]
    lu = spl.splu(s.A.tocsc())
    u_ref, p_ref, e_ref, _ = kr.minres(s.A, s.B, lambda x: 2.5 * lu.solve(x), kr.diag_inverse(s.mass), f, g, maxsteps=500,
                                       tol=1e-8)
    A, B = hipla.SparseMatrix.from_scipy(s.A), hipla.SparseMatrix.from_scipy(s.B)
    pre = hipla.FastDiagonalizationInverse(A, s.component_ids)
    K = hipla.BlockMatrix([[A, B.T], [B, None]])
    Cm = hipla.BlockMatrix([[2.5 * pre, None], [None, hipla.DiagonalMatrix(1.0 / s.mass)]])
    with contextlib.redirect_stdout(io.StringIO()):
        u, errors = MinRes(mat=K, pre=Cm, rhs=hipla.BlockVector([hipla.Vector.from_numpy(f), hipla.Vector.from_numpy(g)]),
                           maxsteps=500, tol=1e-8, printrates=False)
    assert fused.MinresLoop.last_declined is None
    assert len(e_ref) != len(o["minres"][2]) or not np.allclose(e_ref, o["minres"][2])      # (the scale matters)
    check_against(dict(o, scaled=(u_ref, p_ref, np.asarray(e_ref))), "scaled", u[0].numpy(), u[1].numpy(),
                  np.asarray(errors))
    # the scale is a field of the state: a zero (a cleared state) is refused before anything is launched
    from hipla.hip_engine import NssError
    rhs = hipla.BlockVector([hipla.Vector(s.n_u), hipla.Vector(s.n_p)])
    mk = rhs.CreateVector
    loop = fused.MinresLoop.try_create(K, Cm, mk(), (mk(), mk(), mk()), (mk(), mk(), mk()), (mk(), mk()), mk())
    assert loop is not None and loop.state.pre_fdm_scale == 2.5
    loop.state.pre_fdm_scale = 0.0
    with pytest.raises(NssError, match="pre_fdm_scale"):
        loop.enqueue(1, 2)


def test_solve_initial_with_the_inverse(hip_engine):
    from oracle import krylov_ref as kr
    from templates.NavierStokesSIMPLE_iterative import NavierStokes, SyntheticMesh
    with contextlib.redirect_stdout(io.StringIO()):
        ns = NavierStokes(SyntheticMesh(1.0 / 8, dim=3), nu=0.01, inflow="inlet", outflow="outlet", wall="wall|cyl",
                          uin=None, timestep=0.001, order=0)
        ns.SolveInitial(tol=1e-8, maxsteps=500, pre="fdm")
    assert abs(ns.stokes_bpcg_iterations + 1 - 25) <= iteration_tolerance({"iterations": 25}), ns.stokes_bpcg_iterations
    s = ns.system
    f, g = ns.f.vec.numpy(), ns.g.vec.numpy()
    u, p = ns.gfu.numpy(), ns.gfup.numpy()
    lu = spl.splu(s.A.tocsc())
    k = kr.scale_factor(kr.lanczos_ritz(s.A, lu.solve, tol=1e-3))
    _, u_o, p_o, _, _ = kr.bpcg_v2(s.A, s.B, lu.solve, kr.diag_inverse(s.mass), f, g, k, tol=1e-8, maxsteps=500)
    r, d = residuals(s, f, g, u, p)
    r_o, d_o = residuals(s, f, g, u_o, p_o)
    assert r <= 10 * r_o and d <= 10 * d_o, (r, r_o, d, d_o)
    # the velocity of a sparse direct solve of the saddle matrix (the pressure is fixed in its last cell: it is
    # determined up to a constant in the enclosed cavity)
    K = s.saddle_matrix().tocsc()
    keep = np.arange(s.n_u + s.n_p - 1)
    direct = spl.spsolve(K[keep][:, keep], np.concatenate([f, g])[keep])[: s.n_u]
    off, off_o = np.linalg.norm(u - direct), np.linalg.norm(u_o - direct)
    print("velocity against the direct solve: %.3g (oracle %.3g) of %.3g" % (off, off_o, np.linalg.norm(direct)))
    assert off <= 10 * off_o, (off, off_o)


def test_bpcg2_declines_slabs_and_the_condensed_form(hip_engine):
    import hipla
    from hipla.fused import Bpcg2Loop
    from staggered_grid import mac_stokes
    s = mac_stokes(2, 6, 0.01)
    A, B = hipla.SparseMatrix.from_scipy(s.A), hipla.SparseMatrix.from_scipy(s.B)
    pre = hipla.FastDiagonalizationInverse(A, s.component_ids)
    preM = hipla.DiagonalMatrix(1.0 / s.mass)
    BT = B.CreateTranspose()
    assert Bpcg2Loop.try_create(A, B, BT, pre, 1.001, preM, {}, distributed=True) is None
    assert "fast diagonalisation" in Bpcg2Loop.last_declined and "partitioned" in Bpcg2Loop.last_declined
    assert Bpcg2Loop.try_create(A, B, BT, pre, 1.001, preM, {}, condensed=dict(HT=A, H=A, inner=A)) is None
    assert "fast diagonalisation" in Bpcg2Loop.last_declined and "condensed" in Bpcg2Loop.last_declined
    from hipla import fused
    p = fused.native_velocity_pre(1.001 * pre)
    assert p is not None and p.fdm is pre and p.scale == 1.001
    assert fused.ACCEPTS["minres"](p) and fused.ACCEPTS["bpcg1"](p)
    assert not any(fused.ACCEPTS[name](p) for name in ("cg", "partitioned minres", "partitioned bpcg1"))
