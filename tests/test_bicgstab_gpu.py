"""The device-resident BiCGStab loop (csrc/bicgstab.hip) through `hipla.fused.BicgstabLoop` and the C ABI, on operators
no grid produces: A = I + 0.3 R / |R|_inf with R random, 0 to 5 entries per row and some rows empty (nonsymmetric,
condition number below 10), without and with `pre_diag`, n in {1, 2, 63, 64, 65, 257, 1025}.

Bounds.  First iterates: 1e-11 relative to the numpy recurrence (tests/implicit_convection_reference.py) -- rounding
moves an iterate by about 1e-15, a wrong recurrence by O(1); the cap keeps the test from hiding one.  Final residual at
precision 1e-10: |b - A x| <= 10 precision |b| in numpy, after the reference is shown to meet 2 precision |b|.  Identity:
`x == b` with an integer-valued b, for which every sum of the loop is exact (<b, b> = <rhat, v>, so alpha is 1.0)."""

import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

import implicit_convection_reference as icr

pytestmark = pytest.mark.gpu

SIZES = [1, 2, 63, 64, 65, 257, 1025]


def make(eng, A, jacobi=False):
    """(loop, the numpy preconditioner) for the scipy matrix `A`."""
    import hipla
    from hipla.fused import BicgstabLoop
    mat = hipla.SparseMatrix.from_scipy(sp.csr_matrix(A))
    diag = A.diagonal() if jacobi else None
    dinv = None if diag is None else eng.from_host(1.0 / diag)
    return BicgstabLoop(eng, mat, dinv), (None if diag is None else (lambda v: v / diag))


def case(n):
    A = icr.nearly_identity(n, seed=100 + n)
    b = np.random.default_rng(200 + n).standard_normal(n)
    return A, b


def snapshot(eng, loop, x):
    return [eng.to_host(buf).copy() for buf in (x, loop.work["r"], loop.work["p"], loop.hist, loop.scal)]


def test_the_operators_are_what_the_issue_asks_for():
    for n in SIZES[2:]:
        A, _ = case(n)
        lens = np.diff((A - sp.identity(n)).tocsr().indptr)
        assert abs(A - A.T).max() > 0 and np.linalg.cond(A.toarray()) < 10.0 and (lens == 0).any() and lens.max() <= 5


@pytest.mark.parametrize("jacobi", [False, True])
@pytest.mark.parametrize("n", SIZES)
def test_first_iterates_and_final_residual(hip_engine, n, jacobi):
    eng = hip_engine
    A, b = case(n)
    loop, pre = make(eng, A, jacobi)
    bb, x = eng.from_host(b), eng.zeros(n)
    ref_iterates, ref_hist, ref_code = icr.bicgstab(A, b, pre, tol=0.0, maxsteps=3)
    for k in (1, 2, 3):
        k = min(k, n)                                       # (the Krylov space of n <= 2 is exhausted after n iterations)
        count, errors, code = loop.solve(bb, x, 0.0, k)
        # (with the space exhausted the residual is rounding noise and rho' may be exactly zero: a breakdown code then)
        assert count == k and (code == 0 or k == n) and len(errors) == k + 1
        got, want = eng.to_host(x), ref_iterates[k - 1]
        err = np.linalg.norm(got - want) / np.linalg.norm(want)
        print("n = %d, iterate %d: %.3g from the numpy recurrence" % (n, k, err))
        assert err <= 1e-11
        assert errors[0] == pytest.approx(np.linalg.norm(b), rel=1e-14)
        assert np.allclose(errors[1:], ref_hist[:k], rtol=1e-6, atol=1e-13 * errors[0])
    precision = 1e-10
    ref, hist, code = icr.bicgstab(A, b, pre, tol=precision, maxsteps=200)
    norm_b = np.linalg.norm(b)
    assert code == 0 and np.linalg.norm(b - A @ ref[-1]) <= 2.0 * precision * norm_b       # the reference, with room
    count, errors, code = loop.solve(bb, x, precision, 200)
    res = np.linalg.norm(b - A @ eng.to_host(x))
    print("n = %d: %d iterations (numpy %d), |b - A x| / |b| = %.3g" % (n, count, len(hist), res / norm_b))
    assert code == 0 and 0 < count < 200 and abs(count - len(hist)) <= 2
    assert res <= 10.0 * precision * norm_b
    assert errors[-1] < precision * errors[0] and len(errors) == count + 1


@pytest.mark.parametrize("n", SIZES)
def test_identity_takes_one_iteration(hip_engine, n):
    eng = hip_engine
    loop, _ = make(eng, sp.identity(n, format="csr"))
    b = np.random.default_rng(n).integers(-9, 10, size=n).astype(np.float64)
    b[0] = 3.0
    x = eng.from_host(np.full(n, -7.25))
    count, errors, code = loop.solve(eng.from_host(b), x, 1e-8, 50)
    assert (count, code) == (1, 0) and errors[1] == 0.0
    assert np.array_equal(eng.to_host(x), b)


@pytest.mark.parametrize("n", [1, 65, 1025])
def test_zero_right_hand_side_sets_done_at_once(hip_engine, n):
    eng = hip_engine
    A, _ = case(n)
    loop, _ = make(eng, A, True)
    x = eng.from_host(np.full(n, -7.25))
    count, errors, code = loop.solve(eng.zeros(n), x, 1e-8, 20)
    assert (count, code) == (0, 0) and errors == [0.0]
    assert loop.poll() == (True, -1, 0)
    assert np.array_equal(eng.to_host(x), np.zeros(n))


@pytest.mark.parametrize("jacobi", [False, True])
@pytest.mark.parametrize("n", [2, 65, 1025])
def test_a_set_done_word_freezes_the_loop(hip_engine, n, jacobi):
    eng = hip_engine
    A, b = case(n)
    loop, _ = make(eng, A, jacobi)
    x = eng.zeros(n)
    loop.hist = eng.zeros(8)                                # (room for the iterations enqueued below)
    loop.solve(eng.from_host(b), x, 0.0, 1)                 # a live state after one iteration
    loop.ctrl[0] = 1
    before = snapshot(eng, loop, x)
    loop.enqueue(1, 4)
    done, it_final, code = loop.poll()
    assert done and it_final == -1 and code == 0             # (the books of iteration 0 left it_final alone)
    for a, c in zip(before, snapshot(eng, loop, x)):
        assert a.tobytes() == c.tobytes()


def test_the_cap_leaves_done_unset(hip_engine):
    eng = hip_engine
    A, b = case(257)
    loop, _ = make(eng, A)
    x = eng.zeros(257)
    count, errors, code = loop.solve(eng.from_host(b), x, 0.0, 3)
    done, it_final, code = loop.poll()
    assert count == 3 and not done and code == 0 and len(errors) == 4
    last = C.c_int32()
    eng._check(eng.lib.nss_bicgstab_poll(C.byref(loop.state), None, None, C.byref(last), None, eng.stream))
    assert last.value == 2


def test_breakdown_is_a_code(hip_engine):
    import hipla
    eng = hip_engine
    skew = sp.csr_matrix(np.array([[0.0, 1.0], [-1.0, 0.0]]))
    loop, _ = make(eng, skew)
    x = eng.from_host(np.array([5.0, 6.0]))
    count, errors, code = loop.solve(eng.from_host(np.array([1.0, 0.0])), x, 1e-8, 20)
    assert (count, code) == (0, 1) and loop.poll() == (True, -1, 1)
    assert np.array_equal(eng.to_host(x), np.zeros(2))       # the start's x, finite and unchanged
    inv = hipla.BiCGStabSolver(hipla.SparseMatrix.from_scipy(skew), precision=1e-8)
    y = hipla.Vector(2)
    with pytest.raises(FloatingPointError, match="code 1"):
        y.data = inv * hipla.Vector.from_numpy(np.array([1.0, 0.0]))
    assert inv._fused is not None and hipla.fused.BicgstabLoop.last_declined is None
    assert np.isfinite(y.numpy()).all()


def test_solver_takes_the_loop_on_native_operands_and_the_protocol_otherwise(hip_engine):
    import hipla
    A, b = case(257)
    mat = hipla.SparseMatrix.from_scipy(A)
    ref, hist, _ = icr.bicgstab(A, b, lambda v: v / A.diagonal(), tol=1e-10, maxsteps=200)
    out = []
    for enabled in (True, False):
        hipla.fused.ENABLED = enabled
        try:
            inv = hipla.BiCGStabSolver(mat, hipla.DiagonalMatrix(1.0 / A.diagonal()), precision=1e-10)
            x = hipla.Vector(257)
            x.data = inv * hipla.Vector.from_numpy(b)
        finally:
            hipla.fused.ENABLED = True
        assert (inv._fused is not None) == enabled and abs(inv.iterations - len(hist)) <= 2
        assert np.linalg.norm(b - A @ x.numpy()) <= 1e-9 * np.linalg.norm(b)
        out.append(x.numpy())
    assert np.linalg.norm(out[0] - out[1]) <= 1e-9 * np.linalg.norm(out[1])


@pytest.mark.parametrize("what", ["plan_gen", "cap_a", "cap_b"])
def test_stale_state_is_refused_before_any_launch(hip_engine, what):
    eng = hip_engine
    A, b = case(65)
    loop, _ = make(eng, A)
    x = eng.zeros(65)
    loop.hist = eng.zeros(8)                                # (room for the iteration enqueued at the end)
    loop.solve(eng.from_host(b), x, 0.0, 1)
    before = snapshot(eng, loop, x)
    st = loop.state
    keep = getattr(st, what)
    setattr(st, what, keep + 1 if what == "plan_gen" else 1)
    for call in (lambda: eng.lib.nss_bicgstab_iterate(C.byref(st), 1, 2, eng.stream),
                 lambda: eng.lib.nss_bicgstab_start(C.byref(st), loop.work["t"].data_ptr(), 1e-8, eng.stream)):
        assert call() != 0 and b"bicgstab" in eng.lib.nss_last_error()
    setattr(st, what, keep)
    for a, c in zip(before, snapshot(eng, loop, x)):
        assert a.tobytes() == c.tobytes()
    assert eng.lib.nss_bicgstab_iterate(C.byref(st), 1, 2, eng.stream) == 0
