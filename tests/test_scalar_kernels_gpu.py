"""The scalar-transport kernels (csrc/scalar.hip, flux.hip) one at a time, through the C ABI as `hipla.fused.ScalarStepper`
calls it, on operands no grid produces: avg and diff with random, DIFFERENT two-slot rows of 0, 1 or 2 entries, u of
mixed sign with exact zeros, sizes around a workgroup and above one grid-stride pass of the flux kernel (2^20 faces),
the `done` flag, partial arrays on both sides of 4096 (where the summation tree changes its formulation).

References as in tests/test_step_kernels_gpu.py (whose helpers are used): row sums in extended precision rounded once,
1e-13 against the scale of the terms; 1e-15 for the update T + tau delta (one fused
multiply-add against numpy's two roundings: at most one unit in the last place of the terms); bit equality of the
record with the oracle's restatement of the fixed tree."""

import ctypes as C
import itertools
from math import fsum

import numpy as np
import pytest

from oracle import krylov_ref as kr
from test_step_kernels_gpu import SENT, absvec, assert_every_count, flag, matvec, ptr, refused, three_entry_row, two_slot, upload

pytestmark = pytest.mark.gpu

TOL = 1e-13
ONE_PASS = 4096 * 256              # faces of one grid-stride pass of the flux kernel (kScalarFluxBlocks workgroups)
T_REF = 0.375


def flux_case(eng, rng, n_u, n_p, counts=None, buoyant=True, done=None):
    """One launch of nss_scalar_flux_f64 on random operators.  Returns the largest errors of G and f_eff in units of
    their scales (None for f_eff without w_b)."""
    if counts is None:
        avg, dif = two_slot(rng, n_u, n_p), two_slot(rng, n_u, n_p)
        if n_u >= 255:
            assert_every_count(avg)
            assert_every_count(dif)
    else:
        avg, dif = (two_slot(rng, n_u, n_p, [c]) for c in counts)
    u = rng.standard_normal(n_u)
    u[::5] = 0.0                                                   # exact zeros beside both signs
    T, f, w_b = rng.standard_normal(n_p), rng.standard_normal(n_u), rng.standard_normal(n_u)
    tg = eng.from_host(np.concatenate([T, np.full(n_u + 1, SENT)]))        # [T | G | one guard entry]
    g_ptr = tg.data_ptr() + 8 * n_p
    assert n_p % 2 == 1 and g_ptr % 16 == 8                       # the G segment starts on an odd element
    f_eff = eng.from_host(np.full(n_u + 1, SENT))
    bufs = [eng.from_host(x) for x in (u, f, w_b)]
    mats = [upload(eng, avg), upload(eng, dif)]
    stop = None if done is None else flag(eng, done)
    eng._check(eng.lib.nss_scalar_flux_f64(mats[0].handle.ptr, mats[1].handle.ptr, ptr(bufs[2]) if buoyant else None,
                                           ptr(bufs[0]), ptr(bufs[1]), tg.data_ptr(), T_REF, g_ptr,
                                           ptr(f_eff), ptr(stop), eng.stream))
    got, got_f = eng.to_host(tg), eng.to_host(f_eff)
    assert np.array_equal(got[:n_p], T) and got[-1] == SENT and got_f[-1] == SENT
    for buf, host in zip(bufs, (u, f, w_b)):
        assert np.array_equal(eng.to_host(buf), host)
    if done:
        assert (got[n_p:] == SENT).all() and (got_f == SENT).all()
        return 0.0, None
    a, d = matvec(avg, T), matvec(dif, T)
    want = np.asarray(u * a - np.abs(u) * d / 2, dtype=np.float64)
    scale = np.abs(u) * absvec(avg, T) + np.abs(u) * absvec(dif, T) / 2
    err = np.abs(got[n_p:-1] - want)
    assert (err <= TOL * scale).all(), (np.nonzero(err > TOL * scale)[0][:8], err.max())
    assert (got[n_p:-1][u == 0.0] == 0.0).all()
    if n_u >= 255:
        assert (u > 0).any() and (u < 0).any() and (u == 0).any()
        central = np.asarray(u * a, dtype=np.float64)              # without the upwind term
        assert np.linalg.norm(central - want) > 1e-6 * np.linalg.norm(want)
    worst = float(np.max(err[scale > 0] / scale[scale > 0])) if (scale > 0).any() else 0.0
    if not buoyant:
        assert (got_f == SENT).all()                               # the passive scalar writes no f_eff
        return worst, None
    want_f = np.asarray(f + w_b * (a - T_REF), dtype=np.float64)
    scale_f = np.abs(f) + np.abs(w_b) * (absvec(avg, T) + T_REF)
    err_f = np.abs(got_f[:-1] - want_f)
    assert (err_f <= TOL * scale_f).all(), (np.nonzero(err_f > TOL * scale_f)[0][:8], err_f.max())
    return worst, float(np.max(err_f / scale_f))


@pytest.mark.parametrize("buoyant", [True, False])
@pytest.mark.parametrize("n_u", [1, 255, 256, 257, ONE_PASS + 257])
def test_flux_on_random_two_slot_operators(hip_engine, n_u, buoyant):
    """G = u avg - |u| diff / 2 and f_eff = f + w_b (avg - t_ref) to 1e-13 per face, operands untouched, G == 0 where
    u == 0.0; one face: every pair of row lengths; the largest size takes a second grid-stride trip."""
    rng = np.random.default_rng(1000 * (n_u % 9973) + buoyant)
    if n_u == 1:
        errs = [flux_case(hip_engine, rng, 1, 7, counts, buoyant) for counts in itertools.product((0, 1, 2), repeat=2)]
    else:
        errs = [flux_case(hip_engine, rng, n_u, 1001 if n_u > 300 else 7, buoyant=buoyant)]
    print("scalar flux n_u=%d buoyant=%s max err / scale: G %.3e f_eff %s"
          % (n_u, buoyant, max(e[0] for e in errs), max((e[1] for e in errs if e[1] is not None), default=None)))


@pytest.mark.parametrize("buoyant", [True, False])
def test_flux_done_flag_and_clear_flag(hip_engine, buoyant):
    rng = np.random.default_rng(77)
    flux_case(hip_engine, rng, 257, 33, buoyant=buoyant, done=1)   # frozen: outputs untouched
    flux_case(hip_engine, rng, 257, 33, buoyant=buoyant, done=0)   # a flag that is not set changes nothing


def test_flux_refusals_and_no_faces(hip_engine):
    import scipy.sparse as sp
    eng, lib = hip_engine, hip_engine.lib
    rng = np.random.default_rng(5)
    n_u, n_p = 40, 33
    good = [upload(eng, two_slot(rng, n_u, n_p)) for _ in range(2)]
    wide = upload(eng, three_entry_row(rng, n_u, n_p))
    tg = eng.from_host(np.concatenate([rng.standard_normal(n_p), np.full(n_u, SENT)]))
    u, f, w_b, f_eff = (eng.from_host(rng.standard_normal(n_u)) for _ in range(4))
    before = eng.to_host(tg).copy(), eng.to_host(f_eff).copy()
    tail = tg.data_ptr() + 8 * n_p

    def call(avg, dif, w=w_b, force=f, out=f_eff, G=tail):
        return lib.nss_scalar_flux_f64(avg.handle.ptr, dif.handle.ptr, ptr(w), ptr(u), ptr(force), tg.data_ptr(), T_REF, G,
                                       ptr(out), None, eng.stream)
    for pos in range(2):                                            # a three-entry row: an error code, not a fault
        mats = list(good)
        mats[pos] = wide
        refused(eng, call(*mats), "more than two entries")
    refused(eng, call(good[0], upload(eng, two_slot(rng, n_u + 1, n_p))), "differ in shape")
    refused(eng, call(*good, force=None), "w_b without")
    refused(eng, call(*good, out=None), "w_b without")
    refused(eng, call(*good, G=tg.data_ptr()), "aliases")
    refused(eng, lib.nss_scalar_flux_f64(None, None, None, None, None, None, 0.0, None, None, None, None), "scalar_flux")
    bare = [upload(eng, sp.csr_matrix((3, 0))) for _ in range(2)]  # faces but no cells: T has no element 0
    refused(eng, call(*bare), "no columns")
    empty = [upload(eng, sp.csr_matrix((0, n_p))) for _ in range(2)]
    assert call(*empty) == 0, lib.nss_last_error()
    eng.synchronize()
    assert np.array_equal(eng.to_host(tg), before[0]) and np.array_equal(eng.to_host(f_eff), before[1])


# ---- nss_scalar_update_f64 / nss_scalar_record_f64 ----------------------------------------------------------------
def workspace(eng, n):
    count = C.c_int64()
    eng._check(eng.lib.nss_scalar_workspace(n, C.byref(count)))
    return count.value


def record_of(eng, partials, n, c0, slot=1, done=None):
    record = eng.from_host(np.full(3, SENT))
    stop = None if done is None else flag(eng, done)
    eng._check(eng.lib.nss_scalar_record_f64(partials.data_ptr(), n, c0, record.data_ptr(), slot, ptr(stop), eng.stream))
    return eng.to_host(record)


@pytest.mark.parametrize("n", [1, 255, 257, 70001, 4097 * 256 - 5])
def test_update_partials_and_record(hip_engine, n):
    """T += tau delta to 1e-15; partials[b] = <w, T> over workgroup b's 256 cells to 1e-13; the record c0 - sum equals
    the oracle's restatement of the fixed tree on the device's partials bit for bit (4097 partials: the loop
    formulation of the tree, fewer: the all-loads-first one)."""
    eng = hip_engine
    rng = np.random.default_rng(n)
    T, delta, w = rng.standard_normal(n), rng.standard_normal(n), rng.standard_normal(n)
    tau, c0 = 0.05, 1.75
    count = workspace(eng, n)
    assert count == (n + 255) // 256
    t_buf, d_buf, w_buf = eng.from_host(np.append(T, SENT)), eng.from_host(delta), eng.from_host(w)
    partials = eng.from_host(np.full(count + 1, SENT))
    eng._check(eng.lib.nss_scalar_update_f64(n, tau, d_buf.data_ptr(), t_buf.data_ptr(), w_buf.data_ptr(),
                                             partials.data_ptr(), count, None, eng.stream))
    got = eng.to_host(t_buf)
    assert got[-1] == SENT and np.array_equal(eng.to_host(d_buf), delta)
    new = got[:-1]
    assert (np.abs(new - (T + tau * delta)) <= 1e-15 * (np.abs(T) + tau * np.abs(delta))).all()
    part = eng.to_host(partials)
    assert part[-1] == SENT
    prod, mag = w * new, np.abs(w * new)
    pad = (-n) % 256
    want = np.array([fsum(row) for row in np.append(prod, np.zeros(pad)).reshape(-1, 256)])
    scale = np.array([fsum(row) for row in np.append(mag, np.zeros(pad)).reshape(-1, 256)])
    assert (np.abs(part[:-1] - want) <= TOL * scale).all()
    rec = record_of(eng, partials, count, c0)
    assert rec[0] == SENT and rec[2] == SENT
    assert rec[1] == c0 - kr.fixed_sum_1024(part[:-1])
    assert abs(rec[1] - (c0 - fsum(prod))) <= TOL * (abs(c0) + fsum(mag))
    # without a weight vector: the update alone
    t2 = eng.from_host(T)
    eng._check(eng.lib.nss_scalar_update_f64(n, tau, d_buf.data_ptr(), t2.data_ptr(), None, None, 0, None, eng.stream))
    assert np.array_equal(eng.to_host(t2), new)
    # frozen: nothing moves
    t3, p3 = eng.from_host(T), eng.from_host(np.full(count, SENT))
    eng._check(eng.lib.nss_scalar_update_f64(n, tau, d_buf.data_ptr(), t3.data_ptr(), w_buf.data_ptr(), p3.data_ptr(),
                                             count, flag(eng, 1).data_ptr(), eng.stream))
    assert np.array_equal(eng.to_host(t3), T) and (eng.to_host(p3) == SENT).all()
    assert (record_of(eng, partials, count, c0, done=1) == SENT).all()


@pytest.mark.parametrize("n", [0, 1, 64, 1025, 4095, 4096, 4097, 8193, 35000])
def test_record_equals_the_fixed_tree_bit_for_bit(hip_engine, n):
    """nss_scalar_record_f64 on partial arrays of both sides of every change of shape of `fixed_sums_1024`."""
    rng = np.random.default_rng(300 + n)
    x = rng.standard_normal(n) * 10.0 ** rng.integers(-3, 4, size=n)
    partials = hip_engine.from_host(np.append(x, 1e300))          # (the entry behind the end is not summed)
    for c0 in (0.0, -2.5):
        rec = record_of(hip_engine, partials, n, c0, slot=0)
        assert rec[0] == c0 - kr.fixed_sum_1024(x) and rec[1] == SENT


def test_update_and_record_refusals(hip_engine):
    eng, lib = hip_engine, hip_engine.lib
    a, b, w, p = (eng.from_host(np.ones(600)) for _ in range(4))
    refused(eng, lib.nss_scalar_update_f64(600, 0.1, ptr(a), ptr(b), ptr(w), None, 0, None, eng.stream), "go together")
    refused(eng, lib.nss_scalar_update_f64(600, 0.1, ptr(a), ptr(b), None, ptr(p), 3, None, eng.stream), "go together")
    refused(eng, lib.nss_scalar_update_f64(600, 0.1, ptr(a), ptr(b), ptr(w), ptr(p), 2, None, eng.stream), "fewer entries")
    refused(eng, lib.nss_scalar_update_f64(600, 0.1, ptr(a), ptr(a), None, None, 0, None, eng.stream), "scalar_update")
    refused(eng, lib.nss_scalar_record_f64(None, 0, 0.0, None, 0, None, eng.stream), "scalar_record")
    refused(eng, lib.nss_scalar_record_f64(ptr(p), 3, 0.0, ptr(a), -1, None, eng.stream), "scalar_record")
    refused(eng, lib.nss_scalar_workspace(-1, None), "scalar_workspace")
    eng.synchronize()
    assert (eng.to_host(b) == 1.0).all() and (eng.to_host(p) == 1.0).all()
