"""Host logic of the vector layer (hipla/vector.py) on the numpy checker engine: which launches a statement
decomposes into, and what it refuses.

The element-wise kernels read their operands and write the destination in one launch, so an operand may share memory
with the destination only as the very same storage (element i on element i).  The checker engine forms the right-hand
side first and gives right values whatever it is handed; on the GPU a partly overlapping operand is a race between
workgroups that may pass by luck.  So the call pattern is what these tests pin: a spy on the engine asserts that no
operand of `lincomb` overlaps the destination unless it is the same buffer, and records every launch."""

import numpy as np
import pytest

import vector_reference as vr


class Spy:
    """Records (entry point, number of terms) of every call the vector layer makes and checks lincomb's operands."""

    def __init__(self, eng, monkeypatch):
        self.calls = []
        inner = {name: getattr(eng, name) for name in ("lincomb", "scal", "copy", "fill", "zeros", "csr_spmv")}

        def lincomb(dst, terms):
            for _, b in terms:
                assert eng.same_buffer(dst, b) or not eng.overlaps(dst, b), \
                    "lincomb operand overlaps the destination without being the same storage"
            self.calls.append(("lincomb", len(terms)))
            inner["lincomb"](dst, terms)

        def wrap(name):
            def call(*args):
                self.calls.append((name, 0))
                return inner[name](*args)
            return call

        monkeypatch.setattr(eng, "lincomb", lincomb, raising=False)
        for name in ("scal", "copy", "fill", "zeros", "csr_spmv"):
            monkeypatch.setattr(eng, name, wrap(name), raising=False)

    def take(self):
        calls, self.calls = self.calls, []
        return calls


@pytest.mark.parametrize("shift", vr.OVERLAP_SHIFTS)
def test_partly_overlapping_operands_never_reach_lincomb(numpy_engine, monkeypatch, shift):
    import hipla
    n = vr.OVERLAP_N
    rng = np.random.default_rng(shift)
    x0, y0 = vr.small_ints(rng, n), vr.small_ints(rng, n)
    spy = Spy(numpy_engine, monkeypatch)
    for name, run, ref in vr.overlap_statements(n, shift):
        X, Y = hipla.Vector.from_numpy(x0), hipla.Vector.from_numpy(y0)
        x, y = x0.copy(), y0.copy()
        spy.take()
        run(X, Y)                                            # the spy asserts inside
        ref(x, y)
        calls = spy.take()
        assert ("zeros", 0) in calls and ("copy", 0) in calls, (name, calls)      # through one temporary
        np.testing.assert_array_equal(X.numpy(), x, err_msg=name)
        np.testing.assert_array_equal(Y.numpy(), y0, err_msg=name)


def test_statements_without_overlap_issue_the_launches_they_always_did(numpy_engine, monkeypatch):
    """No temporary, no extra launch where no operand overlaps the destination or where it IS the destination."""
    import hipla
    n = 37
    rng = np.random.default_rng(0)
    h = [rng.standard_normal(n) for _ in range(6)]
    W, A, B, C, D, E = (hipla.Vector.from_numpy(v) for v in h)
    P = hipla.Vector.from_numpy(rng.standard_normal(3 * n))
    spy = Spy(numpy_engine, monkeypatch)

    def launches(statement):
        spy.take()
        statement()
        return spy.take()

    def assign(dst, expr):
        dst.data = expr

    def add(dst, expr):
        dst.data += expr

    L = "lincomb"
    a, b, c, d, e = h[1:]
    w = h[0]
    for statement, want_launches, value in (
            (lambda: assign(W, 2.0 * A - 0.5 * B + 3.0 * C), [(L, 3)], lambda w: 2 * a - 0.5 * b + 3 * c),
            (lambda: assign(W, A + B + C - W), [(L, 4)], lambda w: a + b + c - w),         # exact aliasing: in place
            (lambda: assign(W, 2.0 * W), [(L, 1)], lambda w: 2 * w),
            (lambda: assign(W, 0.5 * W + A + 0.25 * W), [(L, 2)], lambda w: 0.75 * w + a),  # the two W terms merged
            (lambda: add(W, 0.75 * A), [(L, 2)], lambda w: w + 0.75 * a),
            (lambda: add(W, A + B + C + D), [(L, 4), (L, 2)], lambda w: w + a + b + c + d),
            (lambda: add(W, A - 2.0 * W), [(L, 2)], lambda w: a - w),                      # x += c x: one assignment
            (lambda: assign(W, A + B + C + D + E), [(L, 1), (L, 4), (L, 2)], lambda w: a + b + c + d + e)):
        assert launches(statement) == want_launches
        w = value(w)
        np.testing.assert_allclose(W.numpy(), w, rtol=1e-13, atol=1e-13)
    # views of one pool that do not touch each other, and a view that is the destination itself
    p = P.numpy()
    assert launches(lambda: assign(P[0:n], P[n:2 * n] + 2.0 * P[2 * n:3 * n])) == [(L, 2)]
    p[0:n] = p[n:2 * n] + 2.0 * p[2 * n:3 * n]
    assert launches(lambda: add(P[1:n], P[n + 1:2 * n])) == [(L, 2)]
    p[1:n] = p[1:n] + p[n + 1:2 * n]
    assert launches(lambda: assign(P[3:n + 3], 3.0 * P[3:n + 3] - P[n + 3:2 * n + 3])) == [(L, 2)]
    p[3:n + 3] = 3.0 * p[3:n + 3] - p[n + 3:2 * n + 3]
    np.testing.assert_allclose(P.numpy(), p, rtol=1e-13, atol=1e-13)
    # block vectors: component by component, the same launches
    U2, V2 = hipla.BlockVector([A, B]), hipla.BlockVector([C, D])
    assert launches(lambda: assign(U2, 2.0 * V2 - U2)) == [(L, 2), (L, 2)]
    assert launches(lambda: add(U2, 0.5 * V2)) == [(L, 2), (L, 2)]
    np.testing.assert_allclose(U2.numpy(), np.concatenate([2.5 * c - a, 2.5 * d - b]), rtol=1e-13, atol=1e-13)


def test_random_view_statements_match_numpy_and_never_race(numpy_engine, monkeypatch):
    import hipla
    rng = np.random.default_rng(2024)
    spy = Spy(numpy_engine, monkeypatch)
    for k in range(120):
        n = int(rng.choice(vr.STATEMENT_SIZES[:4]))
        m, _, _ = vr.statement_matrix(n)
        M = hipla.SparseMatrix.from_scipy(m)
        pool = vr.spread(rng, vr.pool_length(n))
        P = hipla.Vector.from_numpy(pool)
        statement = vr.random_statement(rng, n)
        vr.run_statement(P, M, n, statement)                 # the spy asserts inside
        ref, S = vr.statement_reference(pool, n, statement)
        dest = statement[1]
        got = P.numpy()
        assert np.all(np.abs(got[dest:dest + n] - ref) <= 1e-12 * S + 1e-300), (k, statement)
        want = pool.copy()
        want[dest:dest + n] = got[dest:dest + n]
        np.testing.assert_array_equal(got, want, err_msg=str((k, statement)))    # nothing else moved
    assert any(name == "csr_spmv" for name, _ in spy.calls) and any(name == "copy" for name, _ in spy.calls)


def test_block_components_resolve_their_own_overlap(numpy_engine, monkeypatch):
    import hipla
    n = 300
    rng = np.random.default_rng(5)
    p0, q0 = vr.small_ints(rng, n + 2), vr.small_ints(rng, 7)
    spy = Spy(numpy_engine, monkeypatch)
    for mode in ("=", "+="):
        P, Q = hipla.Vector.from_numpy(p0), hipla.Vector.from_numpy(q0)
        dst = hipla.BlockVector([P[2:n + 2], Q])
        src = hipla.BlockVector([P[0:n], Q])                 # component 0 shifted by two, component 1 the same storage
        p, q = p0.copy(), q0.copy()
        if mode == "=":
            dst.data = 3.0 * src
            p[2:n + 2] = 3.0 * p[0:n]
            q = 3.0 * q
        else:
            dst.data += 3.0 * src
            p[2:n + 2] = p[2:n + 2] + 3.0 * p[0:n]
            q = q + 3.0 * q
        np.testing.assert_array_equal(P.numpy(), p)
        np.testing.assert_array_equal(Q.numpy(), q)
    assert sum(name == "copy" for name, _ in spy.calls) == 2


def test_setitem_refuses_what_getitem_refuses(numpy_engine):
    import hipla
    x0 = np.arange(10, dtype=np.float64)
    X, Y = hipla.Vector.from_numpy(x0), hipla.Vector.from_numpy(np.ones(3))
    for key in (slice(None, None, 2), slice(1, 9, 3), slice(None, None, -1)):
        with pytest.raises(IndexError):
            X[key] = 1.0
        with pytest.raises(IndexError):
            X[key]
    with pytest.raises(IndexError):
        X[1:9:3] = Y
    for key in (len(X), -len(X) - 1, 10 ** 6, np.int64(10)):
        with pytest.raises(IndexError):
            X[key] = 7.0
        with pytest.raises(IndexError):
            X[key]
    X[7:3] = 1.0                                             # empty ranges: nothing happens
    X[5:5] = 1.0
    np.testing.assert_array_equal(X.numpy(), x0)
    X[-1] = 5.0                                              # what stays allowed
    X[np.int32(0)] = 4.0
    X[2:4] = 6.0
    X[7:] = Y
    want = x0.copy()
    want[-1], want[0], want[2:4] = 5.0, 4.0, 6.0
    want[7:] = 1.0
    np.testing.assert_array_equal(X.numpy(), want)
    X[:] = 2.0
    np.testing.assert_array_equal(X.numpy(), np.full(10, 2.0))


class _NeverLaunched:
    """An engine whose inner products must not be reached: it stands for a kernel that trusts the lengths it is given."""

    def __init__(self, eng, with_dot_multi):
        self._eng = eng
        if with_dot_multi:
            self.dot_multi = self._launched

    def _launched(self, *args):
        raise AssertionError("an inner product of mismatching lengths reached the engine")

    dot = _launched

    def __getattr__(self, name):
        if name == "dot_multi":
            raise AttributeError(name)
        return getattr(self._eng, name)


@pytest.mark.parametrize("with_dot_multi", [True, False], ids=["dot_multi", "fallback-loop"])
def test_block_inner_product_checks_component_lengths(numpy_engine, with_dot_multi):
    import hipla
    eng = _NeverLaunched(numpy_engine, with_dot_multi)
    assert hasattr(eng, "dot_multi") == with_dot_multi

    def block(sizes):
        return hipla.BlockVector([hipla.Vector(buf=np.ones(s), engine=eng) for s in sizes])

    for a, b in (((5, 3), (5, 2)), ((5, 3), (4, 3)), ((5, 3), (3, 5)), ((0, 4, 4, 4, 4), (0, 4, 4, 4, 5))):
        with pytest.raises(ValueError):
            hipla.InnerProduct(block(a), block(b))
    with pytest.raises(TypeError):
        hipla.InnerProduct(block((5, 3)), block((5, 3, 1)))
    with pytest.raises(ValueError):
        hipla.InnerProduct(hipla.Vector(buf=np.ones(4), engine=eng), hipla.Vector(buf=np.ones(5), engine=eng))
    # matching lengths still go through (on the real checker engine)
    A = hipla.BlockVector([hipla.Vector.from_numpy(np.full(s, 2.0)) for s in (5, 0, 3)])
    assert hipla.InnerProduct(A, A) == 32.0


def test_hip_engine_dot_multi_checks_lengths_before_any_launch():
    """HipEngine.dot_multi takes each length from x alone: the check comes before anything of the library or the
    buffers is touched (called unbound on host arrays: needs no GPU and no library)."""
    from hipla.hip_engine import HipEngine
    for pairs in ([(np.ones(5), np.ones(4))], [(np.ones(3), np.ones(3))] * 4 + [(np.ones(3), np.ones(2))]):
        with pytest.raises(ValueError):
            HipEngine.dot_multi(object(), pairs)
    with pytest.raises(ValueError):
        HipEngine.dot(_Unbound(), np.ones(2), np.ones(1))


class _Unbound:
    def dot_multi(self, pairs):
        from hipla.hip_engine import HipEngine
        return HipEngine.dot_multi(self, pairs)


def test_dot_depth_arithmetic():
    """The restated launch arithmetic of the dot at its own branch points (the derivation of the depth D: _dot_case in
    tests/test_vector_kernels_gpu.py)."""
    assert [vr.dot_blocks(m) for m in (0, 1, 2048, 2049, 4097, vr.DOT_TWO_TRIPS)] == [1, 1, 1, 2, 3, 257]
    assert vr.dot_depth([(2048, True)]) == 4 + 19 and vr.dot_depth([(2048, False)]) == 8 + 19
    assert vr.dot_depth([(2049, True)]) == 3 + 19 and vr.dot_depth([(1, True)]) == 1 + 19
    assert vr.dot_depth([(vr.DOT_TWO_TRIPS, True)]) == 5 + 20 and vr.dot_depth([(vr.DOT_TWO_TRIPS, False)]) == 8 + 20
