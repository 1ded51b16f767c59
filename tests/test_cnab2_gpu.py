"""The second-order IMEX step on the product engine: the extrapolating flux kernels (csrc/flux.hip) through the C ABI
on the random tables of tests/test_limited_convection_gpu.py, the right-hand side over [A | D | B^T], and
`NavierStokes(time_scheme="cnab2").Advance` against tests/cnab2_reference.py (direct solves), against `DoTimeStep`, and
against itself across calls.

Tolerances: DESIGN.md section 3 -- 1e-13 for a kernel against numpy (the momentum forms per row against the scale of
their terms: the twin's scale times |w_new|, plus |w_old| |prev|; the scalar forms norm-wise, as their twins' tests),
1e-13 / 1e-9 / 1e-8 for `temp`, `raw` and what lies behind both converged inner solves."""

import contextlib
import io

import numpy as np
import pytest
import scipy.sparse as sp

from cnab2_reference import Cnab2Reference, smooth_start
from oracle import krylov_ref as kr
from test_limited_convection_gpu import (LIMITERS, SENT, T_REF, TOL, absvec, code, device_stencil, flag, from_stencil,
                                         matvec, operand, ptr, random_stencil, refused, two_slot, upload)

pytestmark = pytest.mark.gpu

AB2 = (1.5, -0.5)
FIRST = (1.0, 0.0)
FORMS = ("twin",) + LIMITERS               # "twin": the donor kernel over avg and diff; the others: the stencil kernel
TIGHT = dict(precision=1e-14, maxsteps=(5000, 20000))


def rel(a, b):
    nb = np.linalg.norm(b)
    return np.linalg.norm(np.asarray(a) - b) / nb if nb else float(np.linalg.norm(a))


def mean_free(p):
    return p - p.mean()


# ---- 1. the momentum forms on random tables -------------------------------------------------------------------------
def momentum_launch(eng, form, tables, u, prev, ext, weights, done=None, ab2=True):
    """One launch of the form's AB2 kernel (or of its twin, which writes to `prev`)."""
    A, avg, dif, d_st, nflux = tables
    lib = eng.lib
    if not ab2:
        if form == "twin":
            return lib.nss_step_flux_f64(A.handle.ptr, avg.handle.ptr, dif.handle.ptr, u, prev, ptr(done), eng.stream)
        return lib.nss_step_flux_limited_f64(A.handle.ptr, d_st.data_ptr(), nflux, code(form), u, prev, ptr(done), eng.stream)
    if form == "twin":
        return lib.nss_step_flux_ab2_f64(A.handle.ptr, avg.handle.ptr, dif.handle.ptr, u, weights[0], weights[1], prev,
                                         ext, ptr(done), eng.stream)
    return lib.nss_step_flux_limited_ab2_f64(A.handle.ptr, d_st.data_ptr(), nflux, code(form), u, weights[0], weights[1],
                                             prev, ext, ptr(done), eng.stream)


def momentum_case(eng, rng, nflux, n_u, adv_counts=None, patterns=None):
    from staggered_grid import limited_flux
    counts = rng.permutation(np.arange(nflux) % 3) if adv_counts is None else np.asarray(adv_counts)
    adv = two_slot(rng, nflux, n_u, counts)
    st, _ = random_stencil(rng, nflux, n_u, patterns)
    u = operand(rng, n_u)
    a = matvec(adv, u)
    scale = absvec(adv, u) * np.where(st >= 0, np.abs(u)[np.maximum(st, 0)], 0.0).sum(axis=1)
    tables = (upload(adv), upload(from_stencil(st, n_u, (0.5, 0.5))), upload(from_stencil(st, n_u, (-1.0, 1.0))),
              device_stencil(eng, st), nflux)
    history = rng.standard_normal(nflux)
    worst = 0.0
    for form in FORMS:
        want = limited_flux(st, a, u, "donor" if form == "twin" else form)
        twin = eng.from_host(np.full(nflux + 1, SENT))
        d_u = eng.from_host(u)
        eng._check(momentum_launch(eng, form, tables, d_u.data_ptr(), twin.data_ptr(), None, None, ab2=False))
        twin = eng.to_host(twin)[:-1]
        for weights, start in ((AB2, history), (FIRST, np.full(nflux, np.nan))):
            buf = eng.from_host(np.concatenate([u, np.full(nflux + 1, SENT)]))      # [u | ext | one guard entry]
            prev = eng.from_host(np.concatenate([start, [SENT]]))                   # [prev | one guard entry]
            ext_ptr = buf.data_ptr() + 8 * n_u
            assert ext_ptr % 16 == 8                                                # n_u is odd
            eng._check(momentum_launch(eng, form, tables, buf.data_ptr(), prev.data_ptr(), ext_ptr, weights))
            got, got_prev = eng.to_host(buf), eng.to_host(prev)
            assert np.array_equal(got[:n_u], u) and got[-1] == SENT and got_prev[-1] == SENT
            assert np.array_equal(got_prev[:-1], twin), form                         # the twin's bits
            ext = got[n_u:-1]
            if weights is FIRST:
                assert np.isfinite(ext).all() and np.array_equal(ext, twin), form    # the history was not read
                continue
            bound = TOL * (1.5 * scale + 0.5 * np.abs(history))
            err = np.abs(ext - (1.5 * want - 0.5 * history))
            assert (err <= bound).all(), (form, np.nonzero(err > bound)[0][:8], err.max())
            worst = max(worst, float(np.max(err[bound > 0] / bound[bound > 0] * TOL)) if (bound > 0).any() else 0.0)
    return worst


@pytest.mark.parametrize("n_u", [7, 1001])
@pytest.mark.parametrize("nflux", [1, 255, 256, 257, 1000])
def test_momentum_forms_on_random_tables(hip_engine, nflux, n_u):
    """nss_step_flux_ab2_f64 and nss_step_flux_limited_ab2_f64 (three limiters): `prev` out bit-equal to the twin
    kernel's output, `ext` to 1e-13 per row for (3/2, -1/2); with (1, 0) and a NaN history `ext` finite and equal to the
    flux; u untouched, the guard entries behind ext and prev kept.  One flux point: all 16 presence patterns, adv rows
    of 0, 1, 2 entries."""
    rng = np.random.default_rng(2000 * nflux + n_u)
    if nflux == 1:
        errs = [momentum_case(hip_engine, rng, 1, n_u, adv_counts=[p % 3], patterns=[p]) for p in range(16)]
    else:
        errs = [momentum_case(hip_engine, rng, nflux, n_u)]
    print("ab2 momentum nflux=%d n_u=%d max err / scale = %.3e" % (nflux, n_u, max(errs)))


# ---- 2. the scalar forms --------------------------------------------------------------------------------------------
def scalar_launch(eng, form, tables, w_b, u, f, T, weights, G_prev, G_ext, b_prev, f_eff, done=None, ab2=True):
    avg, dif, d_st, nface = tables
    lib = eng.lib
    if not ab2:                                    # the twin: G -> G_prev, f_eff -> f_eff
        if form == "twin":
            return lib.nss_scalar_flux_f64(avg.handle.ptr, dif.handle.ptr, w_b, u, f, T, T_REF, G_prev, f_eff, ptr(done),
                                           eng.stream)
        return lib.nss_scalar_flux_limited_f64(d_st.data_ptr(), nface, code(form), w_b, u, f, T, T_REF, G_prev, f_eff,
                                               ptr(done), eng.stream)
    tail = (w_b, u, f, T, T_REF, weights[0], weights[1], G_prev, G_ext, b_prev, f_eff, ptr(done), eng.stream)
    if form == "twin":
        return lib.nss_scalar_flux_ab2_f64(avg.handle.ptr, dif.handle.ptr, *tail)
    return lib.nss_scalar_flux_limited_ab2_f64(d_st.data_ptr(), nface, code(form), *tail)


def scalar_case(eng, rng, nface, n_p, buoyant, forms=FORMS, patterns=None):
    from staggered_grid import limited_flux
    st, _ = random_stencil(rng, nface, n_p, patterns)
    T = operand(rng, n_p)
    u, f, w_b, hist_G, hist_b = (rng.standard_normal(nface) for _ in range(5))
    if nface > 1:
        u[nface // 2] = 0.0
    tables = (upload(from_stencil(st, n_p, (0.5, 0.5))), upload(from_stencil(st, n_p, (-1.0, 1.0))),
              device_stencil(eng, st), nface)
    d_u, d_f, d_w = eng.from_host(u), eng.from_host(f), eng.from_host(w_b)
    w_ptr, f_ptr = (d_w.data_ptr(), d_f.data_ptr()) if buoyant else (None, None)
    lo = np.where(st[:, 1] >= 0, T[np.maximum(st[:, 1], 0)], 0.0)
    hi = np.where(st[:, 2] >= 0, T[np.maximum(st[:, 2], 0)], 0.0)
    want_b = w_b * (0.5 * (lo + hi) - T_REF)
    errs = []
    for form in forms:
        want = limited_flux(st, u, T, "donor" if form == "twin" else form)
        d_T = eng.from_host(T)
        twin, twin_f = eng.from_host(np.full(nface, SENT)), eng.from_host(np.full(nface, SENT))
        eng._check(scalar_launch(eng, form, tables, w_ptr, d_u.data_ptr(), f_ptr, d_T.data_ptr(), None, twin.data_ptr(),
                                 None, None, twin_f.data_ptr() if buoyant else None, ab2=False))
        twin, twin_f = eng.to_host(twin), eng.to_host(twin_f)
        for weights, start_G, start_b in ((AB2, hist_G, hist_b), (FIRST, np.full(nface, np.nan), np.full(nface, np.nan))):
            tg = eng.from_host(np.concatenate([T, np.full(nface + 1, SENT)]))        # [T | G_ext | one guard entry]
            G_prev, b_prev = (eng.from_host(np.concatenate([x, [SENT]])) for x in (start_G, start_b))
            f_eff = eng.from_host(np.full(nface + 1, SENT))
            g_ptr = tg.data_ptr() + 8 * n_p
            assert g_ptr % 16 == 8
            eng._check(scalar_launch(eng, form, tables, w_ptr, d_u.data_ptr(), f_ptr, tg.data_ptr(), weights,
                                     G_prev.data_ptr(), g_ptr, b_prev.data_ptr() if buoyant else None,
                                     f_eff.data_ptr() if buoyant else None))
            got, got_G, got_b, got_f = (eng.to_host(x) for x in (tg, G_prev, b_prev, f_eff))
            assert np.array_equal(got[:n_p], T) and got[-1] == SENT
            assert got_G[-1] == SENT and got_b[-1] == SENT and got_f[-1] == SENT
            assert np.array_equal(eng.to_host(d_u), u) and np.array_equal(eng.to_host(d_f), f)
            assert np.array_equal(got_G[:-1], twin), form                            # the twin's bits
            ext = got[n_p:-1]
            if nface > 1:
                assert got_G[nface // 2] == 0.0
            if weights is FIRST:
                assert np.isfinite(ext).all() and np.array_equal(ext, twin), form
            else:
                errs.append(rel(ext, 1.5 * want - 0.5 * hist_G))
            if not buoyant:                                                          # the passive form touches neither
                same = np.array_equal(got_b[:-1], start_b, equal_nan=True)
                assert same and (got_f == SENT).all()
                continue
            errs.append(rel(got_b[:-1], want_b))
            if weights is FIRST:
                assert np.isfinite(got_f[:-1]).all()
                errs.append(rel(got_f[:-1], f + want_b))
                errs.append(rel(got_f[:-1], twin_f))                                 # the twin's f_eff, to rounding
            else:
                errs.append(rel(got_f[:-1], f + 1.5 * want_b - 0.5 * hist_b))
    assert max(errs) < TOL, errs
    return max(errs)


@pytest.mark.parametrize("buoyant", [False, True])
@pytest.mark.parametrize("n_p", [7, 1001])
@pytest.mark.parametrize("nface", [1, 255, 256, 257, 1000])
def test_scalar_forms_on_random_tables(hip_engine, nface, n_p, buoyant):
    """nss_scalar_flux_ab2_f64 and nss_scalar_flux_limited_ab2_f64 (three limiters), passive and buoyant: `G_prev` out
    bit-equal to the twin's G, `G_ext`, `b_prev` and `f_eff` (= f_step) to 1e-13 for (3/2, -1/2); with (1, 0) and NaN
    histories everything finite, G_ext equal to the flux and f_eff to the twin's; T, u and f untouched, the guards
    kept, the passive form touching neither b_prev nor f_eff.  One face: all 16 presence patterns."""
    rng = np.random.default_rng(3000 * nface + n_p + int(buoyant))
    if nface == 1:
        errs = [scalar_case(hip_engine, rng, 1, n_p, buoyant, patterns=[p]) for p in range(16)]
    else:
        errs = [scalar_case(hip_engine, rng, nface, n_p, buoyant)]
    print("ab2 scalar nface=%d n_p=%d buoyant=%s max rel err = %.3e" % (nface, n_p, buoyant, max(errs)))


def test_scalar_forms_second_grid_stride_trip(hip_engine):
    """2^20 + 300 faces: 300 lanes make a second trip through the 4096-workgroup grid (the donor kernel and van Leer,
    buoyant)."""
    rng = np.random.default_rng(21)
    print(scalar_case(hip_engine, rng, 2 ** 20 + 300, 1001, True, forms=("twin", "vanleer")))


# ---- 3. refusals, empty input, the done flag ------------------------------------------------------------------------
def test_refusals_empty_input_and_done_flag(hip_engine):
    eng = hip_engine
    rng = np.random.default_rng(5)
    n_u, nflux, n_p = 33, 40, 21
    stop, go = flag(eng, 1), flag(eng, 0)
    st, _ = random_stencil(rng, nflux, n_u)
    d_st = device_stencil(eng, np.concatenate([st, st]))          # (room behind the rows for the misaligned view)
    adv = upload(two_slot(rng, nflux, n_u))
    avg, dif = upload(from_stencil(st, n_u, (0.5, 0.5))), upload(from_stencil(st, n_u, (-1.0, 1.0)))
    host = np.concatenate([rng.standard_normal(n_u), np.full(nflux + 1, SENT)])
    phost = rng.standard_normal(nflux)
    buf, prev = eng.from_host(host), eng.from_host(phost)
    tail = buf.data_ptr() + 8 * n_u
    wide = two_slot(rng, nflux, n_u).tolil()
    wide[nflux // 2, :3] = [1.0, 2.0, 3.0]
    wide = upload(wide.tocsr())
    narrow = upload(two_slot(rng, nflux, n_u))
    eng.csr_narrow_f32(narrow.handle)
    empty = upload(sp.csr_matrix((0, n_u)))

    for form, word in (("twin", "step_flux_ab2"), ("minmod", "step_flux_limited_ab2")):
        def step(mat=adv, stencil=d_st, rows=nflux, u=buf.data_ptr(), p=prev.data_ptr(), e=tail, done=None, w=AB2,
                 mats=None, lim=form):
            a2, d2 = mats if mats is not None else (avg, dif)
            return momentum_launch(eng, lim, (mat, a2, d2, stencil, rows), u, p, e, w, done)
        refused(eng, step(u=None), word)
        refused(eng, step(p=None), word)
        refused(eng, step(e=None), word)
        refused(eng, step(e=prev.data_ptr()), word)                 # ext aliases prev
        refused(eng, step(e=buf.data_ptr()), word)                  # ext aliases u
        refused(eng, step(p=buf.data_ptr() + 8 * (n_u - 1)), word)  # prev overlaps the last entry of u
        refused(eng, step(p=tail + 8), word)                        # prev overlaps ext
        refused(eng, step(mat=wide), word)
        refused(eng, step(mat=narrow), word)
        if form == "twin":
            refused(eng, step(mats=(avg, upload(sp.csr_matrix((nflux, n_u + 1))))), word)
        else:
            refused(eng, step(rows=nflux - 1), word)
            refused(eng, step(rows=nflux + 1), word)
            view = d_st.view(-1)
            refused(eng, step(stencil=view[1:]), word)
            refused(eng, step(stencil=view[2:]), word)
            for lim in (-1, 3):
                rc = eng.lib.nss_step_flux_limited_ab2_f64(adv.handle.ptr, d_st.data_ptr(), nflux, lim, buf.data_ptr(), 1.5,
                                                           -0.5, prev.data_ptr(), tail, None, eng.stream)
                refused(eng, rc, word)
        bare = upload(sp.csr_matrix((3, 0)))                        # rows but no columns: u has no element 0
        refused(eng, step(mat=bare, mats=(bare, bare), rows=3), "no columns")
        assert np.array_equal(eng.to_host(buf), host) and np.array_equal(eng.to_host(prev), phost)      # nothing ran
        assert step(mat=empty, mats=(empty, empty), rows=0) == 0, eng.lib.nss_last_error()
        assert step(done=stop) == 0
        assert np.array_equal(eng.to_host(buf), host) and np.array_equal(eng.to_host(prev), phost)      # done: nothing
        assert step(done=go) == 0
        with_zero = eng.to_host(buf).copy(), eng.to_host(prev).copy()
        assert not (with_zero[0][n_u:-1] == SENT).any() and with_zero[0][-1] == SENT
        assert not np.array_equal(with_zero[1], phost)
        eng.upload(host, buf)
        eng.upload(phost, prev)
        assert step() == 0
        assert np.array_equal(eng.to_host(buf), with_zero[0]) and np.array_equal(eng.to_host(prev), with_zero[1])
        eng.upload(host, buf)
        eng.upload(phost, prev)
    assert eng.lib.nss_step_flux_ab2_f64(None, None, None, None, 1.0, 0.0, None, None, None, None) != 0
    assert eng.lib.nss_step_flux_limited_ab2_f64(None, None, 0, 0, None, 1.0, 0.0, None, None, None, None) != 0

    sst, _ = random_stencil(rng, nflux, n_p)
    d_sst = device_stencil(eng, np.concatenate([sst, sst]))
    savg, sdif = upload(from_stencil(sst, n_p, (0.5, 0.5))), upload(from_stencil(sst, n_p, (-1.0, 1.0)))
    thost = np.concatenate([rng.standard_normal(n_p), np.full(nflux + 1, SENT)])
    tg = eng.from_host(thost)
    u, f, w = (eng.from_host(rng.standard_normal(nflux)) for _ in range(3))
    hosts = [rng.standard_normal(nflux), rng.standard_normal(nflux), np.full(nflux, SENT)]
    G_prev, b_prev, f_eff = (eng.from_host(x) for x in hosts)
    G = tg.data_ptr() + 8 * n_p

    def untouched():
        return np.array_equal(eng.to_host(tg), thost) and all(np.array_equal(eng.to_host(b), h)
                                                               for b, h in zip((G_prev, b_prev, f_eff), hosts))

    for form, word in (("twin", "scalar_flux_ab2"), ("vanleer", "scalar_flux_limited_ab2")):
        def scalar(stencil=d_sst, rows=nflux, w_b=w, vel=u, force=f, T=tg.data_ptr(), gp=G_prev, ge=G, bp=b_prev,
                   out=f_eff, done=None, mats=(savg, sdif)):
            return scalar_launch(eng, form, mats + (stencil, rows), ptr(w_b), ptr(vel), ptr(force), T, AB2, ptr(gp), ge,
                                 ptr(bp), ptr(out), done)
        refused(eng, scalar(vel=None), word)
        refused(eng, scalar(T=None), word)
        refused(eng, scalar(gp=None), word)
        refused(eng, scalar(ge=None), word)
        refused(eng, scalar(force=None), word)                      # w_b without f
        refused(eng, scalar(out=None), word)                        # w_b without f_eff
        refused(eng, scalar(bp=None), word)                         # w_b without b_prev
        refused(eng, scalar(ge=tg.data_ptr()), word)                # G_ext aliases T
        refused(eng, scalar(ge=u.data_ptr()), word)                 # ... u
        refused(eng, scalar(ge=G_prev.data_ptr()), word)            # ... G_prev
        refused(eng, scalar(gp=u), word)
        refused(eng, scalar(gp=tg), word)
        refused(eng, scalar(bp=G_prev), word)
        refused(eng, scalar(out=b_prev), word)
        refused(eng, scalar(out=u), word)
        refused(eng, scalar(out=tg), word)
        if form == "twin":
            refused(eng, scalar(mats=(savg, upload(sp.csr_matrix((nflux, n_p + 1))))), word)
            bare = upload(sp.csr_matrix((3, 0)))                    # faces but no cells: T has no element 0
            refused(eng, scalar(mats=(bare, bare), rows=3), "no columns")
        else:
            refused(eng, scalar(rows=-1), word)
            refused(eng, scalar(stencil=d_sst.view(-1)[1:]), word)
        assert untouched()
        if form == "twin":
            none = upload(sp.csr_matrix((0, n_p)))
            assert scalar(mats=(none, none), rows=0) == 0, eng.lib.nss_last_error()
        else:
            assert scalar(rows=0) == 0, eng.lib.nss_last_error()
        assert scalar(done=stop) == 0
        assert untouched()
        assert scalar(done=go) == 0
        got = [eng.to_host(b).copy() for b in (tg, G_prev, b_prev, f_eff)]
        assert not (got[0][n_p:-1] == SENT).any() and got[0][-1] == SENT and not (got[3] == SENT).any()
        for b, h in zip((tg, G_prev, b_prev, f_eff), [thost] + hosts):
            eng.upload(h, b)
        assert scalar() == 0
        assert all(np.array_equal(eng.to_host(b), g) for b, g in zip((tg, G_prev, b_prev, f_eff), got))
        for b, h in zip((tg, G_prev, b_prev, f_eff), [thost] + hosts):
            eng.upload(h, b)
        assert scalar(w_b=None, force=None, out=None, bp=None) == 0     # the passive form needs none of them
        assert np.array_equal(eng.to_host(b_prev), hosts[1]) and np.array_equal(eng.to_host(f_eff), hosts[2])
        for b, h in zip((tg, G_prev), (thost, hosts[0])):
            eng.upload(h, b)
    for lim in (-1, 3):
        rc = eng.lib.nss_scalar_flux_limited_ab2_f64(d_sst.data_ptr(), nflux, lim, None, u.data_ptr(), None, tg.data_ptr(),
                                                     T_REF, 1.5, -0.5, G_prev.data_ptr(), G, None, None, None, eng.stream)
        refused(eng, rc, "scalar_flux_limited_ab2")


# ---- 4. the right-hand side over [A | D | B^T] ----------------------------------------------------------------------
def mass_of(s):
    return np.full(s.n_u, s.h ** s.dim)


@pytest.mark.parametrize("case", ["3d-inflated", "2d-inflated", "2d-plain", "3d-plain"])
def test_right_hand_side_over_three_blocks(hip_engine, case):
    """temp = f - A u - D F_ext - B^T q from ONE launch of nss_step_rhs_f64 over [A | D | B^T] and the operand
    [u | F_ext | q], with F_ext = 3/2 F(u) - 1/2 F_prev from the extrapolating flux launch: both to 1e-13, plain systems
    and inflated ones; the "cnab2" stepper holds no [A | D]."""
    import hipla
    from hipla.stepping import TimeStepper
    from staggered_grid import mac_stokes
    dim = int(case[0])
    s = mac_stokes(dim, 9 if dim == 3 else 14, 0.01)
    if case.endswith("inflated"):
        s = s.inflate(3)
    A, B = hipla.SparseMatrix.from_scipy(s.A), hipla.SparseMatrix.from_scipy(s.B)
    rng = np.random.default_rng(8)
    f, u0, q0 = rng.standard_normal(s.n_u), rng.standard_normal(s.n_u), rng.standard_normal(s.n_p)
    shared = {}
    st = TimeStepper.try_create(s, A, B, hipla.Vector.from_numpy(f), 0.05, mass_of(s), shared=shared, time_scheme="cnab2")
    assert st is not None, TimeStepper.last_declined
    assert "ADBt" in shared and "mhalf" in shared and "AD" not in shared and "mstar" not in shared
    assert st.AD.width == s.n_u + st.nflux + s.n_p and st.uf.numel() == st.AD.width
    cops = s.convection_operators()
    adv, avg, dif = cops["adv"] @ u0, cops["avg"] @ u0, cops["diff"] @ u0
    flux = adv * avg - 0.5 * np.abs(adv) * dif
    before = rng.standard_normal(st.nflux)
    hip_engine.upload(u0, st.u)
    hip_engine.upload(q0, st.q)
    hip_engine.upload(before, st.F_prev)
    st.weights = AB2
    st.right_hand_side()
    got = hip_engine.to_host(st.uf)
    assert np.array_equal(got[:s.n_u], u0) and np.array_equal(got[s.n_u + st.nflux:], q0)
    want_ext = 1.5 * flux - 0.5 * before
    terms = (f, s.A @ u0, cops["div"] @ want_ext, s.B.T @ q0)
    want = terms[0] - terms[1] - terms[2] - terms[3]
    errs = (rel(got[s.n_u:s.n_u + st.nflux], want_ext), rel(hip_engine.to_host(st.F_prev), flux),
            rel(hip_engine.to_host(st.temp), want))
    print(case, errs)
    assert np.linalg.norm(want) > 0.1 * max(np.linalg.norm(t) for t in terms)       # no cancellation hides an error
    assert max(errs) < 1e-13


# ---- 5. Advance ------------------------------------------------------------------------------------------------------
TAU = 0.05
WALLS = {"x-": 1.0, "x+": 0.0}
GRIDS = {"2d": (2, 8, (0.0, 2.0)), "3d": (3, 5, (0.0, 2.0, -1.0))}


def scalar_args(grid):
    return dict(kappa=0.8, dirichlet=WALLS, buoyancy=GRIDS[grid][2], t_ref=0.5)


def fresh(grid, convection="vanleer", buoyant=True, time_scheme="cnab2"):
    """Converged inner solvers in the statements, a seeded divergence-free start (max |u| tau / h about 0.1), a seeded
    force and start pressure, optionally a buoyant scalar."""
    import hipla
    from templates.NavierStokesSIMPLE_iterative import NavierStokes, SyntheticMesh
    dim, n, _ = GRIDS[grid]
    ns = NavierStokes(SyntheticMesh(1.0 / n, dim=dim), nu=0.01, inflow="inlet", outflow="outlet", wall="wall|cyl",
                      uin=None, timestep=TAU, order=0, convection=convection, time_scheme=time_scheme)
    s = ns.system
    assert s.block_size == 1 and s.n == n
    ns.f.vec.data = hipla.Vector.from_numpy(0.5 * s.h ** s.dim * np.random.default_rng(8).standard_normal(s.n_u))
    u0 = 0.2 * kr.project(s.B, mass_of(s), np.random.default_rng(2).standard_normal(s.n_u))[0]
    ns.gfu.data = hipla.Vector.from_numpy(u0)
    p0 = np.random.default_rng(4).standard_normal(s.n_p)
    ns.gfup.data = hipla.Vector.from_numpy(0.01 * (p0 - p0.mean()))
    if buoyant:
        ns.AddScalar(initial=np.random.default_rng(6).random(s.n_p), precision=1e-14, maxsteps=5000, **scalar_args(grid))
    ops = ns._time_stepping_operators()
    ops["invproj"] = hipla.CGSolver(ops["Lp"], pre=hipla.JacobiPreconditioner(ops["Lp"]), precision=1e-14, maxsteps=20000)
    if time_scheme == "cnab2":
        half = ns._cnab2_operators()
        half["invmhalf"] = hipla.CGSolver(half["mhalf"], pre=hipla.JacobiPreconditioner(half["mhalf"]), precision=1e-14,
                                          maxsteps=5000)
    return ns


def reference_of(ns, grid, buoyant):
    sc = dict(scalar_args(grid), convection=ns._scalar.convection) if buoyant else None
    return Cnab2Reference(ns.system, ns.timestep, ns.gfu.numpy(), ns.f.vec.numpy(), ns.convection, "cnab2", scalar=sc,
                          T0=ns.temperature.numpy() if buoyant else None, q0=ns.gfup.numpy())


def steps(ns, count):
    with contextlib.redirect_stdout(io.StringIO()):
        for _ in range(count):
            ns.DoTimeStep()


def state(ns, buoyant=True):
    return [ns.gfu.numpy(), mean_free(ns.gfup.numpy())] + ([ns.temperature.numpy()] if buoyant else []) + \
        [ns.F_prev.numpy()] + ([ns.G_prev.numpy(), ns.b_prev.numpy()] if buoyant else [])


@pytest.mark.parametrize("buoyant", [False, True])
@pytest.mark.parametrize("inner_pre", ["jacobi", "amg"])
@pytest.mark.parametrize("grid", ["2d", "3d"])
def test_one_step_against_the_reference(hip_engine, grid, inner_pre, buoyant):
    """Advance(1) with converged inner solves, then a second Advance(1) (the weights (3/2, -1/2), the history and q
    handed over by the object) against the reference stage by stage: F_ext, G_ext, f_step, temp and temp_T to 1e-13 on
    the first step, raw and delta to 1e-9, everything behind the solves -- and every stage of the second step -- to
    1e-8."""
    ns = fresh(grid, buoyant=buoyant)
    ref = reference_of(ns, grid, buoyant)
    eng = hip_engine
    for k in (1, 2):
        want = ref.step()
        rec = ns.Advance(1, inner_pre=inner_pre, **TIGHT)
        assert rec.declined is None and ns.advance_declined is None and rec.time_scheme == "cnab2"
        st = ns._steppers[inner_pre]
        errs = dict(F_ext=rel(eng.to_host(st.F), want["F_ext"]), temp=rel(eng.to_host(st.temp), want["temp"]),
                    raw=rel(eng.to_host(st.raw), want["raw"]), temp2=rel(eng.to_host(st.temp2), want["temp2"]),
                    u=rel(ns.gfu.numpy(), want["u"]), q=rel(mean_free(ns.gfup.numpy()), mean_free(want["q"])),
                    F_prev=rel(ns.F_prev.numpy(), want["F"]))
        if buoyant:
            ss = ns._scalar.steppers[inner_pre]
            errs.update(G_ext=rel(eng.to_host(ss.G), want["G_ext"]), f_step=rel(eng.to_host(ss.f_eff), want["f_step"]),
                        temp_T=rel(eng.to_host(ss.temp), want["temp_T"]), delta=rel(eng.to_host(ss.delta), want["delta"]),
                        T=rel(ns.temperature.numpy(), want["T"]), G_prev=rel(ns.G_prev.numpy(), want["G"]),
                        b_prev=rel(ns.b_prev.numpy(), want["b"]))
        print(grid, inner_pre, buoyant, k, errs, rec.mstar_iterations, rec.proj_iterations)
        for key, err in errs.items():
            behind = key in ("temp2", "u", "q", "T")
            bound = 1e-8 if k == 2 or behind else 1e-9 if key in ("raw", "delta") else 1e-13
            assert err < bound, (k, key, err, bound)
        assert abs(rec.div_norm[0] - np.linalg.norm(ns.system.B @ ns.gfu.numpy())) <= 1e-9 * np.linalg.norm(ns.gfu.numpy())
    assert ns._history.valid == {"momentum": True, "scalar": buoyant}


@pytest.mark.parametrize("grid", ["2d", "3d"])
def test_five_steps_against_do_time_step(hip_engine, grid):
    """Advance(5) against five `DoTimeStep`s on a twin, and two `DoTimeStep`s followed by Advance(3) on a third object:
    u, q (mean free), T and the three histories to 1e-8."""
    ns, twin, mixed = fresh(grid), fresh(grid), fresh(grid)
    rec = ns.Advance(5, **TIGHT)
    steps(twin, 5)
    steps(mixed, 2)
    rec_mixed = mixed.Advance(3, **TIGHT)
    assert rec.declined is None and rec_mixed.declined is None
    assert np.abs(twin.gfu.numpy()).max() * TAU / ns.system.h < 0.5
    for other in (ns, mixed):
        errs = [rel(a, b) for a, b in zip(state(other), state(twin))]
        print(grid, errs)
        assert max(errs) < 1e-8, errs
    euler = fresh(grid, time_scheme="euler")
    euler.Advance(5, **TIGHT)
    assert rel(euler.gfu.numpy(), ns.gfu.numpy()) > 1e-4                             # (another scheme: another answer)
    steps(ns, 1)                                                                      # ... and back to the statements
    steps(twin, 1)
    assert max(rel(a, b) for a, b in zip(state(ns), state(twin))) < 1e-8


@pytest.mark.parametrize("buoyant", [False, True])
def test_split_advance_is_bit_identical(hip_engine, buoyant):
    """Advance(2) followed by Advance(3) gives the bits of Advance(5): the history and q are handed over exactly, and
    after `ResetTimeHistory` the next call starts with (1, 0) again (its bits differ)."""
    one, two, three = (fresh("2d", buoyant=buoyant) for _ in range(3))
    one.Advance(5, **TIGHT)
    two.Advance(2, **TIGHT)
    two.Advance(3, **TIGHT)
    for a, b in zip(state(one, buoyant), state(two, buoyant)):
        assert np.array_equal(a, b)
    assert np.array_equal(one.gfup.numpy(), two.gfup.numpy())
    three.Advance(2, **TIGHT)
    three.ResetTimeHistory()
    three.Advance(3, **TIGHT)
    assert rel(three.gfu.numpy(), one.gfu.numpy()) > 1e-7


def test_declined_flux_kernel_declines_the_device_step(hip_engine):
    """Convection operators the flux kernel refuses (here: recorded as refused in the object's shared dict, since no grid
    of the package produces such rows) decline the whole "cnab2" device step with a reason, and the statements run: the
    bits of two `DoTimeStep`s, history and accumulated pressure included."""
    ns, twin = fresh("2d"), fresh("2d")
    ops, half = ns._time_stepping_operators(), ns._cnab2_operators()
    why = "adv: a row holds 3 entries (the row-per-lane kernels take two)"
    ns._stepper_shared = dict(mstar=ops["mstar"], Lp=ops["Lp"], C=ops["correct"], mhalf=half["mhalf"], flux_declined=why)
    rec = ns.Advance(2, **TIGHT)
    steps(twin, 2)
    assert rec.declined == ns.advance_declined and "cnab2" in rec.declined and why in rec.declined
    assert rec.time_scheme == "cnab2" and len(rec.mstar_iterations) == 2 and (rec.scalar_iterations > 0).all()
    for a, b in zip(state(ns), state(twin)):
        assert np.array_equal(a, b)
    assert np.array_equal(ns.gfup.numpy(), twin.gfup.numpy())


@pytest.fixture(scope="module")
def fine_16():
    """The CPU reference's 1280-step state at T = 0.2 on the n = 16 cavity (van Leer), and the start field."""
    from staggered_grid import mac_stokes
    s = mac_stokes(2, 16, 0.01)
    u0 = smooth_start(s)
    return u0, Cnab2Reference(s, 0.2 / 1280, u0, np.zeros(s.n_u), "vanleer").run(1280).u


def test_second_order_on_the_device(hip_engine, fine_16):
    """2-D n = 16, nu = 0.01, T = 0.2, van Leer, smooth start with max |u| = 1: Advance with 10 / 20 / 40 steps and
    precision = 1e-12 against the reference's 1280-step run.  Both ratios are at least 3.5 (the reference itself:
    4.09 and 4.02, tests/test_cnab2_cpu.py)."""
    import hipla
    from templates.NavierStokesSIMPLE_iterative import NavierStokes, SyntheticMesh
    u0, fine = fine_16
    errs = []
    for nsteps in (10, 20, 40):
        ns = NavierStokes(SyntheticMesh(1.0 / 16, dim=2), nu=0.01, inflow="inlet", outflow="outlet", wall="wall|cyl",
                          uin=None, timestep=0.2 / nsteps, order=0, convection="vanleer", time_scheme="cnab2")
        assert ns.system.n == 16 and ns.system.n_u == u0.size
        ns.f.vec.data = hipla.Vector.from_numpy(np.zeros(u0.size))
        ns.gfu.data = hipla.Vector.from_numpy(u0)
        rec = ns.Advance(nsteps, precision=1e-12, maxsteps=(5000, 20000), diagnostics=False)
        assert rec.declined is None
        errs.append(rel(ns.gfu.numpy(), fine))
    print("device errors", errs, errs[0] / errs[1], errs[1] / errs[2])
    assert errs[0] / errs[1] >= 3.5 and errs[1] / errs[2] >= 3.5


def test_default_object_holds_nothing_of_the_scheme(hip_engine):
    """A default ("euler") object after Advance with a buoyant scalar: no history, no AB2 buffer, no [A | D | B^T], no
    half-step operator; a "cnab2" one holds those and no [A | D]."""
    ns = fresh("2d", time_scheme="euler")
    rec = ns.Advance(2)
    st, ss = ns._steppers["jacobi"], ns._scalar.steppers["jacobi"]
    assert rec.declined is None and rec.time_scheme == "euler" and st.time_scheme == "euler"
    assert ns.F_prev is None and ns.G_prev is None and ns.b_prev is None and ns._history is None
    assert ns._stepping_cnab2 is None
    assert set(ns._stepper_shared) & {"ADBt", "mhalf"} == set() and "mhalf" not in ns._scalar.shared
    for obj in (st, ss):
        assert not any(hasattr(obj, name) for name in ("F_prev", "G_prev", "b_prev", "q_acc"))
    assert not hasattr(st, "q") and st.uf.numel() == st.n_u + st.nflux
    cn = fresh("2d")
    cn.Advance(2)
    st, ss = cn._steppers["jacobi"], cn._scalar.steppers["jacobi"]
    assert {"ADBt", "mhalf"} <= set(cn._stepper_shared) and "AD" not in cn._stepper_shared
    assert "mhalf" in cn._scalar.shared and "mstar" not in cn._scalar.shared
    assert st.uf.numel() == st.n_u + st.nflux + st.n_p and st.F_prev.numel() == st.nflux
    assert ss.G_prev.numel() == ss.n_u and ss.b_prev.numel() == ss.n_u
