"""The device-resident Lanczos loop (csrc/lanczos.hip) step by step through the C ABI -- `hipla.eigen.lanczos_state`,
then nss_lanczos_start / _iterate / _poll -- on the operators and covers of tests/lanczos_reference.py, which no grid
produces: sizes at which tails run, ragged block covers of every fused block size, the covers that fall back to the
five launches, a breakdown at step 1 in which every operation is exact.  Every test asserts through nss_lanczos_form
which form of the step ran.

Bounds.  Every delta_j and gamma_{j+1} within 1e-12 |delta_0| of the long-double recurrence, rh_J and zh_J within
1e-12 relative in the 2-norm: rounding moves them by about 1e-15 (tests/test_lanczos_reference_cpu.py holds the same
form in float64 numpy to 1e-14), a wrong coefficient, mask or ring slot by 1e-2 or more.  Everything else is bit for
bit: the exact breakdown, a preconditioner scaled by a power of two, batch splits, a set stop word, a refused state.

All state vectors are views into longer buffers with 64 sentinel doubles on either side (the alignment of a fresh
allocation is kept); the history is pre-filled with the sentinel.

The one buffer whose content after a breakdown depends on where the batch ended is p, the product's output: the
two-launch step makes the books of step j in the second kernel of step j + 1, after that step's product has been
written, so a breakdown found in the middle of a batch leaves p = A zh_{j+1} where one found by the books kernel at
the end of a batch leaves p = A zh_j.  Nothing reads p after a stop; the exact-breakdown test pins both values."""

import ctypes as C

import numpy as np
import pytest

import lanczos_reference as lr

pytestmark = pytest.mark.gpu

SENTINEL = -7.25
GUARD = 64
CAP = 1e-12


class Loop:
    """One state of the loop with guarded vectors; keeps everything the state points at alive."""

    def __init__(self, eng, A, blocks, start, room, scale=1.0, pre=None):
        import hipla
        from hipla import eigen, fused
        self.eng = eng
        self.mat = A if isinstance(A, hipla.SparseMatrix) else hipla.SparseMatrix.from_scipy(A)
        n = self.n = self.mat.height
        if pre is None:
            pre = hipla.JacobiPreconditioner(self.mat) if blocks is None else hipla.BlockJacobi(self.mat, blocks)
        self.pre = pre if scale == 1.0 else scale * pre
        pa = fused.native_velocity_pre(self.pre)
        assert pa is not None and pa.scale == scale
        self.bases = [eng.from_host(np.full(n + 2 * GUARD, SENTINEL)) for _ in range(6)]
        views = [b[GUARD: GUARD + n] for b in self.bases]
        assert all(v.data_ptr() % 256 == b.data_ptr() % 256 for v, b in zip(views, self.bases))
        self.start = hipla.Vector.from_numpy(np.asarray(start, dtype=np.float64))
        self.work = eigen.lanczos_state(self.mat, pa, self.start, room, vecs=views)
        self.work.hist.fill_(SENTINEL)
        self.state = self.work.state

    def form(self):
        return self.eng.lanczos_form(self.state)

    def begin(self):
        return self.eng.lib.nss_lanczos_start(C.byref(self.state), self.eng.stream)

    def iterate(self, j_begin, j_end):
        return self.eng.lib.nss_lanczos_iterate(C.byref(self.state), j_begin, j_end, self.eng.stream)

    def run(self, *batches):
        assert self.begin() == 0, self.eng.lib.nss_last_error()
        for j_begin, j_end in batches:
            assert self.iterate(j_begin, j_end) == 0, self.eng.lib.nss_last_error()
        return self

    def poll(self):
        stop, j_stop, last = C.c_int32(), C.c_int32(), C.c_int32()
        self.eng._check(self.eng.lib.nss_lanczos_poll(C.byref(self.state), C.byref(stop), C.byref(j_stop), C.byref(last),
                                                      self.eng.stream))
        return stop.value, j_stop.value, last.value

    def hist(self):
        return self.eng.to_host(self.work.hist).copy()

    def vec(self, i):
        """v[0], v[1], v[2], z[0], z[1], p for i = 0 .. 5, without the guards"""
        return self.eng.to_host(self.bases[i])[GUARD: GUARD + self.n].copy()

    def guards_intact(self):
        for b in self.bases:
            host = self.eng.to_host(b)
            if not ((host[:GUARD] == SENTINEL).all() and (host[GUARD + self.n:] == SENTINEL).all()):
                return False
        return True

    def snapshot(self, vectors=range(6), partials=False):
        """the bytes of the vectors (guards included), hist, scal and ctrl [and the dot partials]"""
        bufs = [self.bases[i] for i in vectors] + [self.work.hist, self.work.scal, self.work.ctrl]
        bufs += list(self.work.partials) if partials else []
        return [self.eng.to_host(b).tobytes() for b in bufs]


def expected_form(n, form, fold):
    """2 for block Jacobi over runs that cover every dof with a widest block of 2 .. 8 dofs (at n = 1 the widest block of
    "runs2" has one dof: no symmetric-inverse form), else 5."""
    return 2 if fold == 1 and form.startswith("runs") and n >= 2 else 5


def folds_of(form):
    return (1, 0) if form.startswith("runs") else (1,)


def case_loop(eng, n, form, room, scale=1.0, start=None):
    A, _, start0 = lr.operator(n)
    return Loop(eng, A, lr.blocks_of(n, form), start0 if start is None else start, room, scale)


# ---- a. steps against long double -----------------------------------------------------------------------------------
@pytest.mark.parametrize("n,form,fold", [(n, form, fold) for n, form in lr.CASES for fold in folds_of(form)])
def test_steps_against_long_double(hip_engine, n, form, fold):
    eng = hip_engine
    ref = lr.reference(n, form)
    steps = min(lr.STEPS, n)
    enqueued = steps + 1 if n <= 2 else steps               # (an exhausted Krylov space: room to stop one step late)
    with eng.overrides(lanczos_fold=fold):
        loop = case_loop(eng, n, form, enqueued + 8)
        ran = loop.form()
        assert ran == expected_form(n, form, fold)
        loop.run((0, enqueued))
        stop, j_stop, last = loop.poll()
    hist = loop.hist()
    count = lr.comparable(ref)
    err = lr.worst(hist, ref, count)
    print("lanczos steps: form %d %s n = %d: worst %.3g |delta_0| over %d entries (cap %.0e)"
          % (ran, form, n, err, count, CAP))
    assert count >= 1 and err <= CAP
    if ref.breakdown is None:
        assert (stop, j_stop, last) == (0, 0, steps - 1)
        made = steps
        for name, got, want in (("rh", loop.vec(made % 3), ref.rh), ("zh", loop.vec(3 + made % 2), ref.zh)):
            rel = float(np.linalg.norm(got.astype(lr.LD) - want) / np.linalg.norm(want))
            print("lanczos steps: form %d %s n = %d: %s_%d %.3g relative"
                  % (expected_form(n, form, fold), form, n, name, made, rel))
            assert rel <= CAP
    else:
        assert n <= 2 and stop == 1 and j_stop in (ref.breakdown, ref.breakdown + 1) and last == j_stop
        made = j_stop + 1
    assert (hist[2 * made:] == SENTINEL).all() and not (hist[: 2 * made] == SENTINEL).any()
    blocks = lr.blocks_of(n, form)
    if form == "uncovered":
        outside = np.ones(n, dtype=bool)
        outside[np.concatenate(blocks)] = False
        assert outside[-1] and outside.sum() >= 2
        for i in (3, 4):                                    # both buffers of the z ring
            assert (loop.vec(i)[outside] == 0.0).all()
    assert loop.guards_intact()


# ---- b. exact breakdown at step 1 -----------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["point", "two-launch", "five-launch"])
@pytest.mark.parametrize("n", [70, 1025])
def test_exact_breakdown_at_step_1(hip_engine, n, kind):
    import hipla
    from hipla import eigen
    eng = hip_engine
    A, start, blocks = lr.exact_breakdown(n)
    i, i2, k, k2 = lr.breakdown_dofs(n)
    zh1 = np.zeros(n)
    zh1[[i2, k2]] = 0.25
    want_hist = np.array([1.0, 0.5, 1.0, 0.0])
    with eng.overrides(lanczos_fold=0 if kind == "five-launch" else 1):
        rings = []
        for batches in ([(0, 1), (1, 2)], [(0, 2)], [(0, 5)]):
            loop = Loop(eng, A, None if kind == "point" else blocks, start, 12)
            assert loop.form() == (2 if kind == "two-launch" else 5)
            loop.run(*batches)
            assert loop.poll() == (1, 1, 1), (batches, loop.poll())
            hist = loop.hist()
            assert hist[:4].tobytes() == want_hist.tobytes(), (batches, hist[:4])
            assert (hist[4:] == SENTINEL).all()
            before = loop.snapshot(partials=True)
            assert loop.iterate(5, 8) == 0
            assert loop.snapshot(partials=True) == before and loop.poll() == (1, 1, 1)
            rings.append(loop.snapshot(vectors=range(5)))
            # rh_0, rh_1, rh_2 = 0 and zh_1, zh_2 = 0 (z[0] held zh_0 until step 1 wrote zh_2 over it)
            assert np.array_equal(loop.vec(0), start) and np.array_equal(loop.vec(1), 2.0 * zh1)
            assert not loop.vec(2).any() and not loop.vec(3).any() and np.array_equal(loop.vec(4), zh1)
            # p (see the module's docstring): the two-launch form has formed A zh_2 = 0 before it finds the breakdown in
            # the middle of a batch
            late = kind == "two-launch" and batches == [(0, 5)]
            assert np.array_equal(loop.vec(5), np.zeros(n) if late else A @ zh1), batches
            assert loop.guards_intact()
        assert rings[0] == rings[1] == rings[2]
        mat = hipla.SparseMatrix.from_scipy(A)
        pre = hipla.JacobiPreconditioner(mat) if kind == "point" else hipla.BlockJacobi(mat, blocks)
        for check_every in (1, 2, 5):
            ritz = eigen._native_lanczos(mat, pre, hipla.Vector.from_numpy(start), 1e-3, 50, check_every)
            assert ritz is not None and len(ritz) == 2 and abs(ritz - [0.5, 1.5]).max() <= 1e-15, (check_every, ritz)


# ---- c. scaling by a power of two is exact --------------------------------------------------------------------------
def scaled_bits(unscaled, factor):
    return (factor * unscaled).view(np.uint64)


@pytest.mark.parametrize("form,fold", [(form, fold) for form in lr.forms_at(257) for fold in folds_of(form)])
def test_scaling_the_preconditioner_by_a_power_of_two_scales_every_entry_exactly(hip_engine, form, fold):
    eng = hip_engine
    n, steps = 257, lr.STEPS
    with eng.overrides(lanczos_fold=fold):
        runs = {}
        for scale in (1.0, 4.0, 0.25):
            loop = case_loop(eng, n, form, steps + 8, scale)
            assert loop.form() == expected_form(n, form, fold) and loop.state.pre_scale == scale
            loop.run((0, steps))
            assert loop.poll() == (0, 0, steps - 1) and loop.guards_intact()
            runs[scale] = loop.hist()
    assert lr.worst(runs[1.0], lr.reference(n, form)) <= CAP
    for scale in (4.0, 0.25):
        assert np.array_equal(runs[scale][: 2 * steps].view(np.uint64), scaled_bits(runs[1.0][: 2 * steps], scale)), scale
        assert (runs[scale][2 * steps:] == SENTINEL).all()


class Form:
    def __init__(self, mat):
        self.mat, self.condense = mat, False


def test_scaling_a_multiplicative_mypre_scales_every_entry_exactly(hip_engine):
    """The multiplicative MypreA is applied unscaled and its result scaled by lanczos_scale_kernel, which nothing else
    launches: 4 * MypreA against MypreA over 6 steps."""
    import hipla
    from hipla import eigen
    from staggered_grid import mac_stokes
    from templates.NavierStokesSIMPLE_iterative import MypreA, auxiliary_space_preconditioner
    eng = hip_engine
    s = mac_stokes(3, 6, 0.01)
    A = hipla.SparseMatrix.from_scipy(s.A)
    _, _, aux = auxiliary_space_preconditioner(s)
    pre = MypreA(None, Form(A), s.line_blocks(3), GS=True, aux=aux)
    start = eigen.lanczos_start_values(0, s.n_u)
    steps, runs = 6, {}
    for scale in (1.0, 4.0):
        loop = Loop(eng, A, None, start, steps + 8, scale, pre=pre)
        assert loop.form() == 5 and loop.state.pre_amg and loop.state.pre_bjac and loop.state.pre_scale == scale
        loop.run((0, steps))
        assert loop.poll() == (0, 0, steps - 1) and loop.guards_intact()
        runs[scale] = loop.hist()
    assert np.isfinite(runs[1.0][: 2 * steps]).all() and (runs[1.0][: 2 * steps] > 0).all()
    assert np.array_equal(runs[4.0][: 2 * steps].view(np.uint64), scaled_bits(runs[1.0][: 2 * steps], 4.0))
    assert (runs[4.0][2 * steps:] == SENTINEL).all()
    # ... and the unscaled steps are those of the protocol recurrence with the same operator
    ritz = np.linalg.eigvalsh(np.diag(runs[1.0][0: 2 * steps: 2]) + np.diag(runs[1.0][1: 2 * steps - 1: 2], 1)
                              + np.diag(runs[1.0][1: 2 * steps - 1: 2], -1))
    eigen.NATIVE = False
    try:
        vec = A.CreateColVector()
        vec.set_from(start)
        proto = eigen.lanczos_ritz(A, pre, vec, tol=0.0, maxsteps=steps, check_every=steps)
    finally:
        eigen.NATIVE = True
    np.testing.assert_allclose(ritz, proto, rtol=1e-10)


# ---- d. batch splits change no bit ----------------------------------------------------------------------------------
@pytest.mark.parametrize("form,fold", [("runs4", 1), ("runs4", 0), ("point", 1), ("uncovered", 1)])
@pytest.mark.parametrize("n", [65, 1025])
def test_batch_splits_change_no_bit(hip_engine, n, form, fold):
    eng = hip_engine
    with eng.overrides(lanczos_fold=fold):
        snaps = []
        for batches in ([(0, 8)], [(0, 3), (3, 4), (4, 8)]):
            loop = case_loop(eng, n, form, 16)
            assert loop.form() == expected_form(n, form, fold)
            loop.run(*batches)
            assert loop.poll() == (0, 0, 7)
            snaps.append(loop.snapshot())
    assert snaps[0] == snaps[1]
    assert lr.worst(np.frombuffer(snaps[0][6])[:16], lr.reference(n, form)) <= CAP


# ---- e. freeze ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form,fold", [("runs4", 1), ("runs4", 0), ("point", 1), ("uncovered", 1)])
@pytest.mark.parametrize("n", [65, 1025])
def test_a_set_stop_word_freezes_every_buffer(hip_engine, n, form, fold):
    eng = hip_engine
    with eng.overrides(lanczos_fold=fold):
        loop = case_loop(eng, n, form, 16).run((0, 2))
        assert loop.form() == expected_form(n, form, fold) and loop.poll() == (0, 0, 1)
        loop.work.ctrl[0] = 1
        before = loop.snapshot(partials=True)
        assert loop.iterate(2, 6) == 0
        assert loop.poll() == (1, 0, 1)
        assert loop.snapshot(partials=True) == before
        # a zero start vector: stopped by the start, with j_stop = -1
        loop = case_loop(eng, n, form, 16, start=np.zeros(n))
        assert loop.begin() == 0 and loop.poll() == (1, -1, 0)
        before = loop.snapshot(partials=True)
        assert loop.iterate(0, 3) == 0
        assert loop.poll() == (1, -1, 0) and loop.snapshot(partials=True) == before
        assert (loop.hist() == SENTINEL).all() and loop.guards_intact()


# ---- f. refusals ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fold", [1, 0])
@pytest.mark.parametrize("what", ["plan_gen", "cap_a", "cap_b"])
def test_a_stale_or_short_state_is_refused_before_any_launch(hip_engine, what, fold):
    eng = hip_engine
    n = lr.LARGE                                            # (more than one row block of A: a cap_a of 1 is too small)
    with eng.overrides(lanczos_fold=fold):
        loop = case_loop(eng, n, "runs4", 16).run((0, 1))
        assert loop.form() == expected_form(n, "runs4", fold)
        before = loop.snapshot(partials=True)
        st = loop.state
        keep = getattr(st, what)
        assert what == "plan_gen" or keep >= 2
        setattr(st, what, keep + 1 if what == "plan_gen" else 1)
        for call in (lambda: loop.iterate(1, 2), loop.begin):
            assert call() != 0 and b"lanczos" in eng.lib.nss_last_error()
        assert loop.snapshot(partials=True) == before
        setattr(st, what, keep)
        assert loop.iterate(1, 2) == 0 and loop.poll() == (0, 0, 1)
        assert lr.worst(loop.hist()[:4], lr.reference(n, "runs4")) <= CAP
