"""What tests/test_lanczos_steps_gpu.py relies on, shown without a GPU (tests/lanczos_reference.py).

The GPU test holds every delta_j and gamma_{j+1} of the device loop to 1e-12 |delta_0| of the long-double recurrence.
That fixed cap is sound when the un-normalised form the device runs, evaluated in float64, stays far inside it: here it
is held to 1e-14 |delta_0| for every (n, form) of the GPU test (and n = 3), over the steps compared.  The rest: the
operators and covers are what they are described as, the exact case is exact, and the new reference in float64 is the
oracle's recurrence."""

import numpy as np
import pytest

import lanczos_reference as lr


@pytest.mark.parametrize("n", [3] + lr.SIZES + [lr.LARGE])
def test_the_float64_device_form_stays_within_1e_14_of_long_double(n):
    A, dense, start = lr.operator(n)
    forms = lr.forms_at(n) if n != 3 else ["point", "runs2", "bs1", "strided"]
    for form in forms:
        ref = lr.reference(n, form)
        got = lr.device_form(dense, lr.preconditioner(n, form), start, min(lr.STEPS, n))
        count = lr.comparable(ref)
        err = lr.worst(got.hist, ref, count)
        ratio = float(min(ref.hist[: count // 2, 1], default=np.inf) / abs(ref.hist[0, 0]))
        print("n = %d, %s: %d entries, worst %.3g |delta_0|, smallest gamma_j / |delta_0| = %.3g, breakdown %s / %s"
              % (n, form, count, err, ratio, ref.breakdown, got.breakdown))
        assert count >= 1 and err <= 1e-14
        if n > 3:                                               # no step compared is near a breakdown
            assert (ref.breakdown is None) == (n > 2) and (n <= 2 or ratio > 1e-3)
        if ref.breakdown is not None:                           # the exhausted Krylov space of n <= 3
            assert got.breakdown in (ref.breakdown, ref.breakdown + 1, None)
        else:
            for a, b in ((got.rh, ref.rh), (got.zh, ref.zh)):
                assert np.linalg.norm((a - b).astype(np.float64)) <= 1e-13 * np.linalg.norm(b.astype(np.float64))


def test_the_operators_are_what_the_issue_asks_for():
    for n in lr.SIZES[2:] + [lr.LARGE]:
        A, dense, _ = lr.operator(n)
        assert abs(A - A.T).max() == 0.0
        lens = np.diff(A.indptr) - 1                            # off-diagonal entries per row
        empty = np.flatnonzero(lens == 0)
        assert n / 10 <= empty.size <= n / 4 and (lens > 0).sum() > n / 2, (n, empty.size)
        assert np.array_equal(A[empty].toarray(), np.diag(A.diagonal())[empty])
        d = A.diagonal()
        assert d.min() >= 1.0 and d.max() <= 2.0 and abs(A - np.diag(d)).sum(axis=1).max() <= 0.6 + 1e-12
        for form in lr.forms_at(n):
            blocks = lr.blocks_of(n, form)
            if blocks is not None:
                flat = np.concatenate(blocks)
                assert np.unique(flat).size == flat.size and flat.min() >= 0 and flat.max() < n
                covered = np.zeros(n, dtype=bool)
                covered[flat] = True
                if form == "uncovered":
                    assert not covered[-1] and 0.05 * n <= (~covered).sum() <= 0.2 * n
                else:
                    assert covered.all()
                is_run = all(b == list(range(b[0], b[0] + len(b))) for b in blocks)
                assert is_run == (form != "strided")
            if form.startswith("runs") or form == "bs16":
                bs = int(form.lstrip("runsb"))
                lens_b = [len(b) for b in blocks]
                assert max(lens_b) == bs and min(lens_b) < bs and lens_b.count(bs) >= 1
            if n <= 257:
                P = lr.preconditioner(n, form).astype(np.float64).dense()
                keep = np.ones(n, dtype=bool) if blocks is None or form != "uncovered" else covered
                assert abs(P - P.T).max() <= 1e-15 and not P[~keep].any() and not P[:, ~keep].any()
                ev = np.linalg.eigvals(P[np.ix_(keep, keep)] @ dense[np.ix_(keep, keep)]).real
                assert ev.min() > 0 and ev.max() / ev.min() < 10.0, (n, form, ev.max() / ev.min())


def test_the_refined_inverse_blocks_are_inverses_in_long_double():
    n = 65
    dense = lr.operator(n)[1]
    P = lr.preconditioner(n, "runs8")
    for k, dofs in enumerate(lr.blocks_of(n, "runs8")):
        M = dense[np.ix_(dofs, dofs)].astype(lr.LD)
        X = P.inv[k, : len(dofs), : len(dofs)]
        assert abs(M @ X - np.eye(len(dofs), dtype=lr.LD)).max() <= 8 * np.finfo(lr.LD).eps
        assert not P.inv[k, len(dofs):].any() and not P.inv[k, :, len(dofs):].any()


@pytest.mark.parametrize("n", [70, 1025])
def test_the_exact_breakdown_is_exact(n):
    A, start, blocks = lr.exact_breakdown(n)
    dense = A.toarray()
    i, i2, k, k2 = lr.breakdown_dofs(n)
    assert (i // 2, k2 // 2) == (0, len(blocks) - 1) and ((i2 // 2, k // 2) == (255, 256) or n < 514)
    for P in (lr.BlockInverse(dense, blocks), lr.point_jacobi(dense)):
        assert np.array_equal(P.astype(np.float64).dense(), 0.5 * np.eye(n))
        for scale, want in ((1.0, [1.0, 0.5, 1.0, 0.0]), (4.0, [4.0, 2.0, 4.0, 0.0]), (0.25, [0.25, 0.125, 0.25, 0.0])):
            got = lr.device_form(dense, P.scaled(scale), start, 5)
            assert got.hist.ravel().tolist() == want and got.breakdown == 1
            assert not got.rh.any() and not got.zh.any()
            ref = lr.recurrence(dense, P.scaled(scale), start, 5)
            assert ref.hist.ravel().tolist() == want and ref.breakdown == 1
    assert np.array_equal(np.linalg.eigvalsh(np.array([[1.0, 0.5], [0.5, 1.0]])), [0.5, 1.5])


def test_recurrence_in_float64_is_the_oracle_recurrence(monkeypatch):
    """On mac_stokes(2, 8) with block Jacobi over its line blocks: the tridiagonal the oracle hands to its eigensolver
    against `recurrence(..., dtype=float64)` -- the same statements, a sparse against a dense product."""
    import scipy.linalg
    from oracle import krylov_ref as kr
    from staggered_grid import mac_stokes
    s = mac_stokes(2, 8, 0.01)
    tab = np.asarray(s.line_blocks(2))
    blocks = [[int(d) for d in col if d >= 0] for col in tab.T]
    start = kr.lanczos_start(s.n_u)
    seen = []
    real = scipy.linalg.eigvalsh_tridiagonal

    def spy(diag, off, *a, **k):
        seen.append((np.array(diag), np.array(off)))
        return real(diag, off, *a, **k)

    monkeypatch.setattr(scipy.linalg, "eigvalsh_tridiagonal", spy)
    steps = 12
    ritz = kr.lanczos_ritz(s.A, kr.block_jacobi(s.A, tab), tol=0.0, maxsteps=steps, check_every=steps, start=start)
    assert len(seen) == 1 and len(ritz) == steps
    diag, off = seen[0]
    got = lr.recurrence(s.A.toarray(), lr.BlockInverse(s.A.toarray(), blocks), start, steps, dtype=np.float64)
    assert got.breakdown is None and got.hist.dtype == np.float64
    np.testing.assert_allclose(got.hist[:, 0], diag, rtol=1e-12, atol=0)
    np.testing.assert_allclose(got.hist[: steps - 1, 1], off, rtol=1e-12, atol=0)
