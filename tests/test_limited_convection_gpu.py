"""The second-order limited flux kernels (csrc/flux.hip) through the C ABI on operands a staggered grid never
produces -- random stencil rows with every presence pattern, random two-slot adv rows, slopes forced onto every branch of
the limiters -- and through `hipla.fused.TimeStepper` / `ScalarStepper` / `NavierStokes(convection=)` on grid operands:
against the vectorised `staggered_grid.limited_flux`, the oracle's `do_time_step` with `limited_convection`,
tests/limited_reference.py and `DoTimeStep` itself.

Tolerances: DESIGN.md section 3 -- 1e-13 for a kernel against numpy, measured per row against the scale of its terms
(|adv| |u| of the two adv slots times |q_ll| + |q_lo| + |q_hi| + |q_hh|: both slopes are bounded by twice the smaller
difference, each difference errs by 2^-53 of its two terms, and where the device and numpy disagree on the sign of an
a that is zero to rounding the two branches differ by |a| times such a sum); 1e-9 / 1e-8 behind converged inner solves."""

import contextlib
import io
import itertools

import numpy as np
import pytest
import scipy.sparse as sp

from limited_reference import limited_coupled_step
from oracle import krylov_ref as kr

pytestmark = pytest.mark.gpu

TOL = 1e-13
SENT = -7.25                       # what output buffers hold before a launch
LD = np.longdouble
T_REF = 0.375
LIMITERS = ("donor", "minmod", "vanleer")
TIGHT = dict(precision=1e-14, maxsteps=(5000, 20000))
FIXED = (1.0, 2.0, 3.0, 2.0, 4.0)  # q[0 .. 5): the values the forced rows point at


def matvec(mat, x):
    """mat @ x with every two-entry row summed in extended precision and rounded once."""
    mat = sp.csr_matrix(mat)
    prod = mat.data.astype(LD) * np.asarray(x, dtype=np.float64)[mat.indices].astype(LD)
    out = np.zeros(mat.shape[0], dtype=LD)
    np.add.at(out, np.repeat(np.arange(mat.shape[0]), np.diff(mat.indptr)), prod)
    return np.asarray(out, dtype=np.float64)


def absvec(mat, x):
    mat = sp.csr_matrix(mat)
    return matvec(sp.csr_matrix((np.abs(mat.data), mat.indices, mat.indptr), shape=mat.shape), np.abs(x))


def two_slot(rng, m, n, counts=None):
    """Random (m, n) CSR with 0, 1 or 2 entries per row (a third of the rows each unless `counts` is given), random
    columns, every fourth two-entry row holding the SAME column twice (kept as two entries: no summing of duplicates)."""
    counts = rng.permutation(np.arange(m) % 3) if counts is None else np.asarray(counts)
    indptr = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    cols = rng.integers(0, n, size=int(indptr[-1])).astype(np.int32)
    twice = indptr[:-1][counts == 2][::4]
    cols[twice + 1] = cols[twice]
    mat = sp.csr_matrix((rng.standard_normal(cols.size), cols, indptr), shape=(m, n))
    mat.sort_indices()
    assert mat.nnz == cols.size
    return mat


def random_stencil(rng, rows, n, patterns=None):
    """(rows, 4) int32 with random columns; presence patterns (bit k = column k present) cycle through all 16 unless
    given.  From 64 rows on, three groups of forced rows over FIXED (all four present):
      rows 16 .. 24: (0, 1, 2, 4)   p == q == +1 for a >= 0, == -1 for a < 0
      rows 24 .. 32: (1, 0, 1, 0)   p and q of opposite signs both ways
      rows 32 .. 40: (lo, lo, hi, hi)  p == 0 both ways."""
    st = rng.integers(0, n, size=(rows, 4)).astype(np.int32)
    pat = rng.permutation(np.arange(rows) % 16) if patterns is None else np.asarray(patterns)
    if rows >= 64:
        pat[16:40] = 15
        st[16:24] = (0, 1, 2, 4)
        st[24:32] = (1, 0, 1, 0)
        st[32:40, 0], st[32:40, 3] = st[32:40, 1], st[32:40, 2]
    for k in range(4):
        st[(pat >> k) & 1 == 0, k] = -1
    return st, pat


def operand(rng, n):
    q = rng.standard_normal(n)
    q[:5] = FIXED
    return q


def device_stencil(eng, st):
    return eng.torch.from_numpy(np.ascontiguousarray(st, dtype=np.int32)).to(eng.device)


def from_stencil(st, n, weights):
    """avg / diff of the stencil's (lo, hi) as a two-slot CSR matrix, duplicates kept as two entries."""
    present = st[:, 1:3] >= 0
    indptr = np.concatenate([[0], np.cumsum(present.sum(axis=1))]).astype(np.int32)
    vals = np.broadcast_to(np.asarray(weights, dtype=np.float64), present.shape)[present]
    mat = sp.csr_matrix((vals, st[:, 1:3][present], indptr), shape=(st.shape[0], n))
    assert mat.nnz == int(present.sum())
    mat.sort_indices()
    return mat


def upload(mat):
    import hipla
    return hipla.SparseMatrix.from_scipy(mat)


def flag(eng, value):
    return eng.torch.tensor([value], dtype=eng.torch.int32, device=eng.device)


def ptr(buf):
    return None if buf is None else buf.data_ptr()


def refused(eng, rc, word):
    msg = eng.lib.nss_last_error().decode()
    assert rc != 0 and word in msg, (rc, msg)


def rel(a, b):
    nb = np.linalg.norm(b)
    return np.linalg.norm(a - b) / nb if nb else float(np.linalg.norm(a))


def code(limiter):
    return LIMITERS.index(limiter)


# ---- 1. nss_step_flux_limited_f64 on random tables ----------------------------------------------------------------
def momentum_case(eng, rng, nflux, n_u, limiters=LIMITERS, adv_counts=None, patterns=None):
    """The launches of `limiters` on one set of random tables; returns the largest error in units of the bound's
    scale."""
    from staggered_grid import limited_flux
    zero = nflux // 2
    counts = rng.permutation(np.arange(nflux) % 3) if adv_counts is None else np.asarray(adv_counts)
    if adv_counts is None and nflux > 1:
        counts[zero] = 0                                            # adv == 0.0 exactly: an empty adv row
    adv = two_slot(rng, nflux, n_u, counts)
    st, pat = random_stencil(rng, nflux, n_u, patterns)
    if patterns is None and nflux > 1:
        st[zero], pat[zero] = rng.integers(0, n_u, size=4), 15      # ... beside a full stencil row
        assert zero >= 40 and set(pat) == set(range(16))            # every presence pattern occurs
    u = operand(rng, n_u)
    a = matvec(adv, u)
    scale = absvec(adv, u) * np.where(st >= 0, np.abs(u)[np.maximum(st, 0)], 0.0).sum(axis=1)
    A, d_st = upload(adv), device_stencil(eng, st)
    worst, got_by = 0.0, {}
    for lim in limiters:
        host = np.concatenate([u, np.full(nflux + 1, SENT)])      # [u | F | one guard entry]
        buf = eng.from_host(host)
        flux_ptr = buf.data_ptr() + 8 * n_u
        assert flux_ptr % 16 == 8                                   # n_u is odd: the segment starts on an odd element
        eng._check(eng.lib.nss_step_flux_limited_f64(A.handle.ptr, d_st.data_ptr(), nflux, code(lim), buf.data_ptr(),
                                                     flux_ptr, None, eng.stream))
        got = eng.to_host(buf)
        assert np.array_equal(got[:n_u], u) and got[-1] == SENT
        want = limited_flux(st, a, u, lim)
        err = np.abs(got[n_u:-1] - want)
        assert (err <= TOL * scale).all(), (lim, np.nonzero(err > TOL * scale)[0][:8], err.max())
        if (scale > 0).any():
            worst = max(worst, float(np.max(err[scale > 0] / scale[scale > 0])))
        got_by[lim] = got[n_u:-1]
    if nflux > 1 and adv_counts is None:
        assert (a > 0).any() and (a < 0).any() and a[zero] == 0.0
        for lim in limiters:
            assert got_by[lim][zero] == 0.0
    if nflux >= 64 and set(limiters) == set(LIMITERS):
        donor = got_by["donor"]
        for lim in ("minmod", "vanleer"):
            assert np.linalg.norm(got_by[lim] - donor) > 1e-2 * np.linalg.norm(donor)
        live = np.abs(a[16:40]) > 0
        assert live.any()
        # p == q: both limiters give s = p, F = a (U + p / 2); opposite signs and p == 0: donor cell
        same = slice(16, 24)
        up = np.where(a[same] >= 0, 2.0, 3.0)
        half = np.where(a[same] >= 0, 0.5, -0.5)
        for lim in ("minmod", "vanleer"):
            assert np.abs(got_by[lim][same] - a[same] * (up + half)).max() <= TOL * scale[same].max()
            assert np.array_equal(got_by[lim][24:40], donor[24:40])
        # limiter 0 against nss_step_flux_f64 on avg and diff built from the same stencil
        avg, dif = upload(from_stencil(st, n_u, (0.5, 0.5))), upload(from_stencil(st, n_u, (-1.0, 1.0)))
        buf = eng.from_host(np.concatenate([u, np.full(nflux + 1, SENT)]))
        eng._check(eng.lib.nss_step_flux_f64(A.handle.ptr, avg.handle.ptr, dif.handle.ptr, buf.data_ptr(),
                                             buf.data_ptr() + 8 * n_u, None, eng.stream))
        twin = eng.to_host(buf)[n_u:-1]
        assert (np.abs(twin - donor) <= TOL * scale).all()
    return worst


@pytest.mark.parametrize("n_u", [7, 1001])
@pytest.mark.parametrize("nflux", [1, 255, 256, 257, 1000])
def test_momentum_flux_on_random_tables(hip_engine, nflux, n_u):
    """F = a (U + s / 2) to 1e-13 per row for the three limiters, u untouched, the guard entry kept, adv == 0.0 giving
    exactly 0, the limited results visibly not donor's, the forced rows on their branches, limiter 0 equal to
    nss_step_flux_f64 to the same bound.  One flux point: all 16 presence patterns x adv rows of 0, 1, 2 entries."""
    rng = np.random.default_rng(1000 * nflux + n_u)
    if nflux == 1:
        errs = [momentum_case(hip_engine, rng, 1, n_u, adv_counts=[k], patterns=[p])
                for p, k in itertools.product(range(16), (0, 1, 2))]
    else:
        errs = [momentum_case(hip_engine, rng, nflux, n_u)]
    print("limited flux nflux=%d n_u=%d max err / scale = %.3e" % (nflux, n_u, max(errs)))


# ---- 2. nss_scalar_flux_limited_f64 -------------------------------------------------------------------------------
def scalar_case(eng, rng, nface, n_p, buoyant, limiters=LIMITERS, patterns=None):
    from staggered_grid import limited_flux
    st, _ = random_stencil(rng, nface, n_p, patterns)
    T = operand(rng, n_p)
    u, f, w_b = (rng.standard_normal(nface) for _ in range(3))
    if nface > 1:
        u[nface // 2] = 0.0
    tg = np.concatenate([T, np.full(nface + 1, SENT)])             # [T | G | one guard entry]
    d_st, d_u, d_f, d_w = device_stencil(eng, st), eng.from_host(u), eng.from_host(f), eng.from_host(w_b)
    lo = np.where(st[:, 1] >= 0, T[np.maximum(st[:, 1], 0)], 0.0)
    hi = np.where(st[:, 2] >= 0, T[np.maximum(st[:, 2], 0)], 0.0)
    want_f = f + w_b * (0.5 * (lo + hi) - T_REF)
    errs = []
    for lim in limiters:
        buf, f_eff = eng.from_host(tg), eng.from_host(np.full(nface + 1, SENT))
        g_ptr = buf.data_ptr() + 8 * n_p
        assert g_ptr % 16 == 8
        eng._check(eng.lib.nss_scalar_flux_limited_f64(d_st.data_ptr(), nface, code(lim), ptr(d_w) if buoyant else None,
                                                       ptr(d_u), ptr(d_f), buf.data_ptr(), T_REF, g_ptr, ptr(f_eff),
                                                       None, eng.stream))
        got, got_f = eng.to_host(buf), eng.to_host(f_eff)
        assert np.array_equal(got[:n_p], T) and got[-1] == SENT and got_f[-1] == SENT
        assert np.array_equal(eng.to_host(d_u), u)
        errs.append(rel(got[n_p:-1], limited_flux(st, u, T, lim)))
        if nface > 1:
            assert got[n_p + nface // 2] == 0.0
        if buoyant:
            errs.append(rel(got_f[:-1], want_f))
        else:
            assert (got_f == SENT).all()                            # the passive form writes no f_eff
    assert max(errs) < TOL, errs
    return max(errs)


@pytest.mark.parametrize("buoyant", [False, True])
@pytest.mark.parametrize("n_p", [7, 1001])
@pytest.mark.parametrize("nface", [1, 255, 256, 257, 1000])
def test_scalar_flux_on_random_tables(hip_engine, nface, n_p, buoyant):
    """G and f_eff to 1e-13 (norm-wise) for the three limiters, passive and buoyant; T and u untouched, the guards kept,
    u == 0.0 giving exactly 0.  One face: all 16 presence patterns."""
    rng = np.random.default_rng(1000 * nface + n_p + int(buoyant))
    if nface == 1:
        errs = [scalar_case(hip_engine, rng, 1, n_p, buoyant, patterns=[p]) for p in range(16)]
    else:
        errs = [scalar_case(hip_engine, rng, nface, n_p, buoyant)]
    print("limited scalar flux nface=%d n_p=%d buoyant=%s max rel err = %.3e" % (nface, n_p, buoyant, max(errs)))


def test_scalar_flux_second_grid_stride_trip(hip_engine):
    """2^20 + 257 faces: 257 lanes make a second trip through the 4096-workgroup grid (buoyant van Leer, passive
    minmod)."""
    rng = np.random.default_rng(20)
    nface = 2 ** 20 + 257
    print(scalar_case(hip_engine, rng, nface, 1001, True, limiters=("vanleer",)),
          scalar_case(hip_engine, rng, nface, 1001, False, limiters=("minmod",)))


# ---- 3. refusals, empty input, the done flag -----------------------------------------------------------------------
def test_refusals_empty_input_and_done_flag(hip_engine):
    eng, lib = hip_engine, hip_engine.lib
    rng = np.random.default_rng(5)
    n_u, nflux, n_p = 33, 40, 21
    stop, go = flag(eng, 1), flag(eng, 0)
    adv = upload(two_slot(rng, nflux, n_u))
    st, _ = random_stencil(rng, nflux, n_u)
    d_st = device_stencil(eng, np.concatenate([st, st]))          # (room behind the rows for the misaligned view)
    host = np.concatenate([rng.standard_normal(n_u), np.full(nflux + 1, SENT)])
    buf = eng.from_host(host)
    tail = buf.data_ptr() + 8 * n_u

    def step(mat=adv, stencil=d_st.data_ptr(), rows=nflux, lim=1, u=buf.data_ptr(), flux=tail, done=None):
        return lib.nss_step_flux_limited_f64(mat.handle.ptr if mat is not None else None, stencil, rows, lim, u, flux,
                                             ptr(done), eng.stream)
    word = "step_flux_limited"
    refused(eng, step(mat=None), word)
    refused(eng, step(stencil=None), word)
    refused(eng, step(u=None), word)
    refused(eng, step(flux=None), word)
    refused(eng, step(lim=-1), word)
    refused(eng, step(lim=3), word)
    refused(eng, step(rows=nflux - 1), word)
    refused(eng, step(rows=nflux + 1), word)
    refused(eng, step(stencil=d_st.data_ptr() + 4), word)
    refused(eng, step(stencil=d_st.data_ptr() + 8), word)
    refused(eng, step(flux=buf.data_ptr()), word)
    wide = two_slot(rng, nflux, n_u).tolil()
    wide[nflux // 2, :3] = [1.0, 2.0, 3.0]
    refused(eng, step(mat=upload(wide.tocsr())), word)
    narrow = upload(two_slot(rng, nflux, n_u))
    eng.csr_narrow_f32(narrow.handle)
    refused(eng, step(mat=narrow), word)
    assert np.array_equal(eng.to_host(buf), host)                   # nothing ran
    assert step(mat=upload(sp.csr_matrix((0, n_u))), rows=0) == 0, lib.nss_last_error()
    assert step(done=stop) == 0
    assert np.array_equal(eng.to_host(buf), host)                   # done: nothing written
    assert step(done=go) == 0
    with_zero = eng.to_host(buf).copy()
    assert not (with_zero[n_u:-1] == SENT).any() and with_zero[-1] == SENT
    eng.upload(host, buf)
    assert step() == 0
    assert np.array_equal(eng.to_host(buf), with_zero)              # done = 0 gives the bits of done = NULL

    sst, _ = random_stencil(rng, nflux, n_p)
    d_sst = device_stencil(eng, np.concatenate([sst, sst]))
    thost = np.concatenate([rng.standard_normal(n_p), np.full(nflux + 1, SENT)])
    tg = eng.from_host(thost)
    u, f, w = (eng.from_host(rng.standard_normal(nflux)) for _ in range(3))
    fhost = np.full(nflux, SENT)
    f_eff = eng.from_host(fhost)
    G = tg.data_ptr() + 8 * n_p

    def scalar(stencil=d_sst.data_ptr(), rows=nflux, lim=2, w_b=w, vel=u, force=f, T=tg.data_ptr(), g=G, out=f_eff, done=None):
        return lib.nss_scalar_flux_limited_f64(stencil, rows, lim, ptr(w_b), ptr(vel), ptr(force), T, T_REF, g, ptr(out),
                                               ptr(done), eng.stream)
    word = "scalar_flux_limited"
    refused(eng, scalar(stencil=None), word)
    refused(eng, scalar(vel=None), word)
    refused(eng, scalar(T=None), word)
    refused(eng, scalar(g=None), word)
    refused(eng, scalar(force=None), word)                          # w_b without f
    refused(eng, scalar(out=None), word)                            # w_b without f_eff
    refused(eng, scalar(lim=-1), word)
    refused(eng, scalar(lim=3), word)
    refused(eng, scalar(rows=-1), word)
    refused(eng, scalar(stencil=d_sst.data_ptr() + 4), word)
    refused(eng, scalar(g=tg.data_ptr()), word)
    refused(eng, scalar(g=u.data_ptr()), word)
    refused(eng, scalar(out=u), word)
    refused(eng, scalar(out=tg), word)
    assert np.array_equal(eng.to_host(tg), thost) and np.array_equal(eng.to_host(f_eff), fhost)
    assert scalar(rows=0) == 0, lib.nss_last_error()
    assert scalar(done=stop) == 0
    assert np.array_equal(eng.to_host(tg), thost) and np.array_equal(eng.to_host(f_eff), fhost)
    assert scalar(done=go) == 0
    got, got_f = eng.to_host(tg).copy(), eng.to_host(f_eff).copy()
    assert not (got[n_p:-1] == SENT).any() and got[-1] == SENT and not (got_f == SENT).any()
    eng.upload(thost, tg)
    eng.upload(fhost, f_eff)
    assert scalar() == 0
    assert np.array_equal(eng.to_host(tg), got) and np.array_equal(eng.to_host(f_eff), got_f)
    assert scalar(w_b=None, force=None, out=None) == 0              # the passive form needs neither


# ---- 4. grid operands through the stepper --------------------------------------------------------------------------
def mass_of(s):
    return np.full(s.n_u, s.h ** s.dim)


@pytest.mark.parametrize("scheme", ["minmod", "vanleer"])
@pytest.mark.parametrize("case", ["3d-inflated", "2d-inflated", "2d-plain", "3d-plain"])
def test_flux_and_right_hand_side_against_numpy(hip_engine, case, scheme):
    """After `right_hand_side()` the F part of [u | F] equals `limited_flux` and temp the oracle's temp, both to
    1e-13, on mac_stokes(2, 14), mac_stokes(3, 9) and both inflated x 3; the stepper holds the stencil and neither avg
    nor diff."""
    import hipla
    from hipla.fused import TimeStepper
    from staggered_grid import limited_flux, mac_stokes
    dim = int(case[0])
    s = mac_stokes(dim, 9 if dim == 3 else 14, 0.01)
    if case.endswith("inflated"):
        s = s.inflate(3)
    A, B = hipla.SparseMatrix.from_scipy(s.A), hipla.SparseMatrix.from_scipy(s.B)
    f = np.random.default_rng(8).standard_normal(s.n_u)
    shared = {}
    st = TimeStepper.try_create(s, A, B, hipla.Vector.from_numpy(f), 0.05, mass_of(s), shared=shared, convection=scheme)
    assert st is not None and st.flux_declined is None, (TimeStepper.last_declined, st and st.flux_declined)
    assert st.convection == scheme and st.stencil is shared["stencil"] and "avg" not in shared and "diff" not in shared
    assert np.array_equal(st.stencil.cpu().numpy(), s.convection_stencil())
    u0 = np.random.default_rng(2).standard_normal(s.n_u)
    hip_engine.upload(u0, st.u)
    st.right_hand_side()
    cops = s.convection_operators()
    want_flux = limited_flux(s.convection_stencil(), cops["adv"] @ u0, u0, scheme)
    got = hip_engine.to_host(st.uf)
    assert np.array_equal(got[:s.n_u], u0)
    err_flux = rel(got[s.n_u:], want_flux)
    want = kr.do_time_step(s.A, s.B, mass_of(s), 0.05, u0, f, lambda u: s.limited_convection(u, scheme))["temp"]
    err_temp = rel(hip_engine.to_host(st.temp), want)
    print("flux", err_flux, "temp", err_temp)
    assert err_flux < 1e-13
    assert err_temp < 1e-13
    donor = kr.upwind_convection(cops, u0)
    assert rel(s.limited_convection(u0, scheme), donor) > 1e-2      # (the scheme is visible in the term)


class WideAdv:
    """A system whose `adv` holds one row of three entries (the third an explicit 0.0: the same operator)."""

    def __init__(self, system):
        self._system = system

    def __getattr__(self, name):
        return getattr(self._system, name)

    def convection_operators(self):
        ops = dict(self._system.convection_operators())
        adv = ops["adv"].tocsr()
        row = int(np.argmax(np.diff(adv.indptr) == 2))
        spare = next(c for c in range(adv.shape[1]) if c not in adv.indices[adv.indptr[row]:adv.indptr[row + 1]])
        at = adv.indptr[row + 1]
        indptr = adv.indptr.copy()
        indptr[row + 1:] += 1
        ops["adv"] = sp.csr_matrix((np.insert(adv.data, at, 0.0), np.insert(adv.indices, at, spare), indptr), shape=adv.shape)
        ops["adv"].sort_indices()
        return ops


def test_flux_declined_still_governs_the_fallback(hip_engine):
    """An `adv` row of three entries: the limited stepper reports `flux_declined`, holds no stencil and forms temp
    through `ConvectionOperator` (which evaluates such an operator on the host) -- to 1e-13 of the oracle's."""
    import hipla
    from hipla.fused import TimeStepper
    from staggered_grid import mac_stokes
    from templates.NavierStokesSIMPLE_iterative import ConvectionOperator
    s = mac_stokes(2, 9, 0.01)
    wide = WideAdv(s)
    assert np.diff(wide.convection_operators()["adv"].indptr).max() == 3
    A, B = hipla.SparseMatrix.from_scipy(s.A), hipla.SparseMatrix.from_scipy(s.B)
    f = np.random.default_rng(8).standard_normal(s.n_u)
    st = TimeStepper.try_create(wide, A, B, hipla.Vector.from_numpy(f), 0.05, mass_of(s),
                                conv_operator=lambda: ConvectionOperator(wide, "vanleer"), convection="vanleer")
    assert st is not None and st.flux_declined.startswith("adv") and st.stencil is None and st.convection == "vanleer"
    u0 = np.random.default_rng(2).standard_normal(s.n_u)
    hip_engine.upload(u0, st.u)
    st.right_hand_side()
    want = kr.do_time_step(s.A, s.B, mass_of(s), 0.05, u0, f, lambda u: s.limited_convection(u, "vanleer"))["temp"]
    assert rel(hip_engine.to_host(st.temp), want) < 1e-13


# ---- 5. one step and five steps against the oracle -----------------------------------------------------------------
def fresh(scheme, dim=3, maxh=0.1):
    from templates.NavierStokesSIMPLE_iterative import NavierStokes, SyntheticMesh
    extra = {} if scheme is None else {"convection": scheme}
    ns = NavierStokes(SyntheticMesh(maxh, dim=dim), nu=0.01, inflow="inlet", outflow="outlet", wall="wall|cyl", uin=None,
                      timestep=0.05, order=1, **extra)
    ns.AddForce(np.random.default_rng(8).standard_normal(ns.system.n_u))
    return ns


def start_velocity(s):
    return kr.project(s.B, mass_of(s), np.random.default_rng(2).standard_normal(s.n_u))[0]


def tighten(ns):
    import hipla
    ops = ns._time_stepping_operators()
    ops["invmstar"] = hipla.CGSolver(ops["mstar"], pre=hipla.JacobiPreconditioner(ops["mstar"]), precision=1e-14, maxsteps=5000)
    ops["invproj"] = hipla.CGSolver(ops["Lp"], pre=hipla.JacobiPreconditioner(ops["Lp"]), precision=1e-14, maxsteps=20000)
    return ns


def set_velocity(ns, u):
    import hipla
    ns.gfu.data = hipla.Vector.from_numpy(u)


@pytest.mark.parametrize("scheme", ["minmod", "vanleer"])
@pytest.mark.parametrize("dim", [3, 2])
@pytest.mark.parametrize("inner_pre", ["jacobi", "amg"])
def test_one_step_against_the_oracle(hip_engine, dim, inner_pre, scheme):
    """Advance(1) with converged inner solves against `kr.do_time_step` with conv = `limited_convection`: temp 1e-13,
    unprojected increment 1e-9, projected increment and new velocity 1e-8."""
    ns = fresh(scheme, dim)
    s = ns.system
    u0 = start_velocity(s)
    want = kr.do_time_step(s.A, s.B, mass_of(s), ns.timestep, u0, ns.f.vec.numpy(), lambda u: s.limited_convection(u, scheme))
    set_velocity(ns, u0)
    rec = ns.Advance(1, inner_pre=inner_pre, **TIGHT)
    assert rec.declined is None and ns.advance_declined is None and rec.flux_declined is None
    assert rec.convection == scheme
    st = ns._steppers[inner_pre]
    assert st.stencil is not None
    errs = (rel(hip_engine.to_host(st.temp), want["temp"]), rel(hip_engine.to_host(st.raw), want["temp2_unprojected"]),
            rel(hip_engine.to_host(st.temp2), want["temp2"]), rel(ns.gfu.numpy(), want["u"]))
    print(scheme, inner_pre, dim, errs, rec.mstar_iterations, rec.proj_iterations)
    assert errs[0] < 1e-13
    assert errs[1] < 1e-9
    assert errs[2] < 1e-8
    assert errs[3] < 1e-8


@pytest.mark.parametrize("scheme", ["minmod", "vanleer"])
def test_five_steps_against_do_time_step(hip_engine, scheme):
    """Advance(5) and five DoTimeStep() calls on a twin (its `ConvectionOperator` runs the limited kernel and -D F as
    statements), both with converged inner solves: velocities agree to 1e-8.  Damped force and 1e-2 start field as in
    tests/test_time_stepper_gpu.py: the trajectory stays bounded."""
    import hipla
    ns, twin = fresh(scheme), tighten(fresh(scheme))
    for obj in (ns, twin):
        obj.f.vec.data = hipla.Vector.from_numpy(1e-4 * obj.f.vec.numpy())
    u0 = 1e-2 * start_velocity(ns.system)
    set_velocity(ns, u0)
    set_velocity(twin, u0)
    rec = ns.Advance(5, **TIGHT)
    with contextlib.redirect_stdout(io.StringIO()):
        for _ in range(5):
            twin.DoTimeStep()
    assert twin.conv_operator.scheme == scheme and twin.conv_operator.stencil is not None
    err = rel(ns.gfu.numpy(), twin.gfu.numpy())
    print("five steps", scheme, err, rec.mstar_iterations, rec.proj_iterations, np.abs(ns.gfu.numpy()).max())
    assert np.abs(ns.gfu.numpy()).max() < 1.0
    assert err < 1e-8
    upwind = fresh(None)
    upwind.f.vec.data = hipla.Vector.from_numpy(1e-4 * upwind.f.vec.numpy())
    set_velocity(upwind, u0)
    upwind.Advance(5, **TIGHT)
    assert rel(upwind.gfu.numpy(), ns.gfu.numpy()) > 1e-6           # (the scheme moved the trajectory)


# ---- 6. with a scalar ----------------------------------------------------------------------------------------------
CASES = {"2d": (2, 8, (0.0, 0.5)), "3d": (3, 5, (0.0, 0.5, -0.2))}
WALLS = {"x-": 1.0, "x+": 0.0}


def fresh_scalar(case, scheme=None, scalar=True, buoyant=True, scalar_scheme=None):
    import hipla
    from templates.NavierStokesSIMPLE_iterative import NavierStokes, SyntheticMesh
    dim, n, beta = CASES[case]
    extra = {} if scheme is None else {"convection": scheme}
    ns = NavierStokes(SyntheticMesh(1.0 / n, dim=dim), nu=0.01, inflow="inlet", outflow="outlet", wall="wall|cyl",
                      uin=None, timestep=0.05, order=0, **extra)
    s = ns.system
    assert s.block_size == 1 and s.n == n
    ns.f.vec.data = hipla.Vector.from_numpy(1e-4 * np.random.default_rng(8).standard_normal(s.n_u))
    u0 = 1e-2 * kr.project(s.B, np.full(s.n_u, s.h ** s.dim), np.random.default_rng(2).standard_normal(s.n_u))[0]
    ns.gfu.data = hipla.Vector.from_numpy(u0)
    if scalar:
        ns.AddScalar(0.8, dirichlet=WALLS, buoyancy=beta if buoyant else None, t_ref=0.5,
                     initial=np.random.default_rng(6).random(s.n_p), precision=1e-14, maxsteps=5000,
                     convection=scalar_scheme)
    return ns


@pytest.mark.parametrize("scheme", ["minmod", "vanleer"])
@pytest.mark.parametrize("inner_pre", ["jacobi", "amg"])
@pytest.mark.parametrize("case", ["2d", "3d"])
def test_one_step_with_a_scalar_against_the_reference(hip_engine, case, inner_pre, scheme):
    """Advance(1) with converged inner solves against `limited_coupled_step`: G, f_eff and temp_T to 1e-13, delta to
    1e-9, T, u and the recorded wall flux to 1e-8 (the bounds of tests/test_scalar_transport_gpu.py)."""
    ns = fresh_scalar(case, scheme)
    s = ns.system
    u0, T0, f = ns.gfu.numpy(), ns.temperature.numpy(), ns.f.vec.numpy()
    want = limited_coupled_step(s, ns.timestep, u0, T0, f, kappa=0.8, dirichlet=WALLS, buoyancy=CASES[case][2], t_ref=0.5,
                                convection=scheme)
    rec = ns.Advance(1, inner_pre=inner_pre, **TIGHT)
    assert rec.declined is None and ns.advance_declined is None and rec.flux_declined is None
    st = ns._scalar.steppers[inner_pre]
    assert st.convection == scheme and st.stencil is not None and "avg" not in ns._scalar.shared
    errs = dict(G=rel(hip_engine.to_host(st.G), want["G"]), f_eff=rel(hip_engine.to_host(st.f_eff), want["f_eff"]),
                temp_T=rel(hip_engine.to_host(st.temp), want["temp_T"]), delta=rel(hip_engine.to_host(st.delta), want["delta"]),
                T=rel(ns.temperature.numpy(), want["T"]), u=rel(ns.gfu.numpy(), want["u"]),
                wall=abs(rec.wall_flux[0] - want["wall_flux"]) / abs(want["wall_flux"]))
    print(case, inner_pre, scheme, errs, rec.mstar_iterations, rec.proj_iterations, rec.scalar_iterations)
    assert errs["G"] < 1e-13 and errs["f_eff"] < 1e-13 and errs["temp_T"] < 1e-13
    assert errs["delta"] < 1e-9
    assert errs["T"] < 1e-8 and errs["u"] < 1e-8 and errs["wall"] < 1e-8
    donor = limited_coupled_step(s, ns.timestep, u0, T0, f, kappa=0.8, dirichlet=WALLS, buoyancy=CASES[case][2], t_ref=0.5,
                                 convection="upwind")
    assert rel(want["G"], donor["G"]) > 1e-2


@pytest.mark.parametrize("scheme", ["minmod", "vanleer"])
@pytest.mark.parametrize("case", ["2d", "3d"])
def test_five_steps_with_a_scalar_against_do_time_step(hip_engine, case, scheme):
    """Advance(5) against five `DoTimeStep()` calls on a twin, both with converged solves: T, u and the wall flux to
    1e-8."""
    ns, twin = fresh_scalar(case, scheme), tighten(fresh_scalar(case, scheme))
    rec = ns.Advance(5, **TIGHT)
    walls = []
    with contextlib.redirect_stdout(io.StringIO()):
        for _ in range(5):
            twin.DoTimeStep()
            walls.append(twin._scalar.wall_flux(twin.temperature))
    s = ns.system
    assert np.abs(twin.gfu.numpy()).max() * ns.timestep / s.h < 0.05
    errs = (rel(ns.temperature.numpy(), twin.temperature.numpy()), rel(ns.gfu.numpy(), twin.gfu.numpy()),
            np.abs(rec.wall_flux - np.array(walls)).max() / np.abs(walls).max())
    print(case, scheme, errs, rec.scalar_iterations)
    assert rec.declined is None and rec.convection == scheme and max(errs) < 1e-8


@pytest.mark.parametrize("case", ["2d", "3d"])
def test_upwind_velocity_with_a_limited_passive_scalar(hip_engine, case):
    """Velocity "upwind", scalar "vanleer", no buoyancy: u after Advance(3) is bit for bit the run without a scalar,
    while T moves -- and not as the upwind scalar's T does."""
    ns, free = fresh_scalar(case, buoyant=False, scalar_scheme="vanleer"), fresh_scalar(case, scalar=False)
    donor = fresh_scalar(case, buoyant=False)
    T0 = ns.temperature.numpy()
    rec, rec_free = ns.Advance(3), free.Advance(3)
    donor.Advance(3)
    st = ns._scalar.steppers["jacobi"]
    assert rec.declined is None and rec.convection == "upwind" and st.convection == "vanleer" and st.f_eff is None
    assert ns._steppers["jacobi"].stencil is None and st.stencil is not None
    assert np.array_equal(ns.gfu.numpy(), free.gfu.numpy()) and np.array_equal(ns.gfup.numpy(), free.gfup.numpy())
    assert np.array_equal(rec.kinetic_energy, rec_free.kinetic_energy) and np.array_equal(rec.div_norm, rec_free.div_norm)
    assert rel(ns.temperature.numpy(), T0) > 1e-3
    assert rel(ns.temperature.numpy(), donor.temperature.numpy()) > 1e-6


# ---- 7. the default is untouched -----------------------------------------------------------------------------------
def test_default_objects_hold_no_stencil(hip_engine):
    """A default object's steppers have `stencil is None`, hold avg and diff as before, and record "upwind" (the
    existing suites are the check that their bits did not move)."""
    ns = fresh_scalar("2d")
    rec = ns.Advance(1)
    st, sc = ns._steppers["jacobi"], ns._scalar.steppers["jacobi"]
    assert rec.declined is None and rec.convection == "upwind"
    assert st.convection == "upwind" and st.stencil is None and "stencil" not in ns._stepper_shared
    assert sc.convection == "upwind" and sc.stencil is None and "stencil" not in ns._scalar.shared
    assert st.avg is ns._stepper_shared["avg"] and sc.diff is ns._scalar.shared["diff"]
    assert ns._scalar.stencil is None and ns.conv_operator.stencil is None
