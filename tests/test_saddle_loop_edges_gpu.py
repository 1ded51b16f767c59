"""The three device-resident saddle-point loops (csrc/bpcg2.hip, csrc/bpcg1.hip, csrc/minres.hip) through their Python
entry points, on the systems of tests/saddle_cases.py: sizes at which the scalar tails of bpcg2_k4_kernel,
minres_m3_kernel and minres_m4_kernel run (odd parts, parts shorter than one workgroup or one wave, n_p = 1), solution and
right-hand side 8 bytes off a 16-byte boundary (the instantiations without double2), block-Jacobi blocks no grid makes
(255 ... 513 blocks, a short last block, ragged blocks, a dof in no block), every plan switch, the done word, a zero
right-hand side.  Every test asserts that the fused loop ran.

Bounds (tests/test_saddle_cases_cpu.py holds the oracle to the conditions behind them).
* First iterates: 1e-11 relative to the oracle's iterate -- a reordering moves the oracle's own iterates by less than
  1e-15, a lost tail element or a wrong partial moves an iterate by O(1 / n) or more; histories to rtol 1e-8.
* Convergence at 1e-10: the iteration count within max(3, 3 %) of the oracle's, the solution within 1e-8 relative of the
  dense solve (ten times what the oracle is held to: one iteration apart is one convergence factor apart).
* Plan switches and the poll interval: identical bits.

A block Jacobi that leaves a dof in no block is singular: every iterate stays zero at that dof and the run is the run on
the system without it, which is what the scale factor and the dense solve are taken from (saddle_cases.scale,
dense_solution(keep=)).

MINRES with a block Jacobi that M3 can apply itself has two forms, the apply inside M3 and on its own (minres_fuse);
the stand-alone apply writes its partials of <z_new, v_new> where the fused M3 writes them, so this pair too gives
identical bits."""

import collections
import contextlib
import functools
import io
import re

import numpy as np
import pytest

import saddle_cases as sc

pytestmark = pytest.mark.gpu

SENTINEL = -7.25
Run = collections.namedtuple("Run", "count x hist k")
ids = dict(ids=lambda v: "%dx%d" % v if isinstance(v, tuple) else str(v))


class Form:
    def __init__(self, mat):
        self.mat, self.condense = mat, False


# ---- the preconditioners for A: point Jacobi or block Jacobi over runs of consecutive dofs ---------------------------
def blocks_of(pre, n_u):
    """`pre`: "point", "runs2" (blocks of two dofs, a one-dof last block when n_u is odd), "runs123" (ragged) or
    "runs2-uncovered" (blocks of two, the last dof of an odd n_u in no block)."""
    if pre == "point":
        return None
    if pre == "runs123":
        return sc.runs(n_u, [1, 2, 3])
    blocks = sc.runs(n_u, [2])
    if pre == "runs2-uncovered":
        assert len(blocks[-1]) == 1
        blocks = blocks[:-1]
    return blocks


@functools.lru_cache(maxsize=None)
def host_pre(size, pre):
    from oracle import krylov_ref as kr
    A = sc.case(*size)[0]
    blocks = blocks_of(pre, size[0])
    return kr.jacobi(A) if blocks is None else kr.block_jacobi(A, sc.table(blocks))


@functools.lru_cache(maxsize=None)
def scale_of(size, pre):
    return sc.scale(sc.case(*size)[0], host_pre(size, pre))


@functools.lru_cache(maxsize=None)
def reference(method, size, pre, k, tol, maxsteps):
    """The oracle's run (shared between the tests; read only)."""
    from oracle import krylov_ref as kr
    A, B, f, g, mass = sc.case(*size)
    return Run(*sc.reference(method, (A, B, f, g), host_pre(size, pre), kr.diag_inverse(mass), k, tol, maxsteps), k)


@functools.lru_cache(maxsize=None)
def exact_solution(size, pre):
    A, B, f, g, _ = sc.case(*size)
    keep = np.ones(size[0], dtype=bool)
    if pre == "runs2-uncovered":
        keep[-1] = False
    return sc.dense_solution(A, B, f, g, keep)


# ---- one run of an entry point --------------------------------------------------------------------------------------
def offset_view(values):
    """(`values` as a Range(1, 1 + n) view into a vector of n + 2 entries with a sentinel at both ends, that vector)."""
    import hipla
    host = np.full(values.size + 2, SENTINEL)
    host[1:-1] = values
    base = hipla.Vector.from_numpy(host)
    view = base.Range(1, 1 + values.size)
    assert isinstance(view, hipla.Vector) and view.buf.data_ptr() % 16 == 8
    return view, base


def solve(method, size, pre, tol, maxsteps, offset=False, poll_every=None, rhs=None):
    """`method` through its entry point on the system of `size` with the preconditioner `pre`; BPCG v2 takes its scale
    factor from `scale_of`, the textbook BPCG estimates and prints its own.  `offset`: solution and right-hand side are
    views 8 bytes off a 16-byte boundary, whose sentinels and right-hand sides are checked afterwards.  `rhs`: (f, g)
    instead of the system's.  Returns Run(iterations done, [u; p], history, k)."""
    import hipla
    from hipla import fused
    from bramble_pasciak_cg import bramble_pasciak_cg
    from minres import MinRes
    from solvers.bramblepasciak_new import BpcgSession
    A, B, f, g, mass = sc.case(*size)
    f, g = (f, g) if rhs is None else rhs
    n_u, n_p = size
    Ad, Bd = hipla.SparseMatrix.from_scipy(A), hipla.SparseMatrix.from_scipy(B)
    blocks = blocks_of(pre, n_u)
    preA = hipla.JacobiPreconditioner(Ad) if blocks is None else hipla.BlockJacobi(Ad, blocks)
    preS = hipla.DiagonalMatrix(1.0 / mass)
    bases = []
    if offset:
        # (the textbook BPCG takes `solution` as its start vector: zeros; the other two zero it themselves)
        start = 0.0 if method == "bpcg1" else SENTINEL
        (fv, gv, su, sp_), bases = zip(*(offset_view(v) for v in (f, g, np.full(n_u, start), np.full(n_p, start))))
    else:
        fv, gv = hipla.Vector.from_numpy(f), hipla.Vector.from_numpy(g)
        su, sp_ = hipla.Vector(n_u), hipla.Vector(n_p)
    sol = hipla.BlockVector([su, sp_])
    loop = {"bpcg2": fused.Bpcg2Loop, "bpcg1": fused.Bpcg1Loop, "minres": fused.MinresLoop}[method]
    loop.last_declined = "try_create was not called"
    keep_poll = fused.POLL_EVERY
    fused.POLL_EVERY = poll_every or keep_poll
    out = io.StringIO()
    try:
        with contextlib.redirect_stdout(out):
            if method == "bpcg2":
                k = scale_of(size, pre)
                ses = BpcgSession(Form(Ad), Form(Bd), None, fv, gv, preA, preS, sol=sol, k=k)
                assert ses.fused is not None, ses.fused_declined
                ses.first_direction()
                it, hist, _ = ses.fused.run(ses.wdn, ses.err0, tol, True, maxsteps)
                count, hist = it + 1, np.array(hist)
            elif method == "bpcg1":
                x, errors = bramble_pasciak_cg(Ad, Bd, None, preA, preS, fv, gv, solution=sol, tolerance=tol,
                                               max_steps=maxsteps, print_rates=False)
                assert x is sol
                k = float(re.search(r"scale factor:\s+(\S+)", out.getvalue()).group(1))
                count, hist = len(errors) - (1 if errors[-1] < tol else 0), np.array(errors)
            else:
                k = None
                x, errors = MinRes(mat=hipla.BlockMatrix([[Ad, Bd.T], [Bd, None]]),
                                   pre=hipla.BlockMatrix([[preA, None], [None, preS]]), rhs=hipla.BlockVector([fv, gv]),
                                   sol=sol, maxsteps=maxsteps, tol=tol, printrates=False)
                assert x is sol
                count, hist = len(errors) - 1, np.array(errors)
    finally:
        fused.POLL_EVERY = keep_poll
    assert loop.last_declined is None, (method, size, pre, loop.last_declined)     # the fused loop was taken
    for base, values in zip(bases, (f, g, None, None)):
        host = base.numpy()
        assert host[0] == SENTINEL and host[-1] == SENTINEL, (method, size, "a sentinel was overwritten")
        assert values is None or np.array_equal(host[1:-1], values)
    return Run(count, sol.numpy(), hist, k)


def check_first_iterates(method, size, pre, steps, offset=False):
    """The iterates after `steps` iterations (each capped at what the oracle needs to converge minus one: beyond that
    the Krylov space of the smallest systems is exhausted) within 1e-11 of the oracle's, the histories to rtol 1e-8.
    Returns the largest distance."""
    worst, k = 0.0, None
    for n in sorted(steps):
        if k is not None and n > reference(method, size, pre, k, 1e-10, 500).count - 1:
            break
        got = solve(method, size, pre, 0.0, n, offset=offset)
        k = got.k if method == "bpcg1" else scale_of(size, pre) if method == "bpcg2" else 0.0
        assert n <= reference(method, size, pre, k, 1e-10, 500).count - 1, "no size needs fewer than two iterations"
        want = reference(method, size, pre, k, 0.0, n)
        err = sc.distance(got.x, want.x)
        print("FIRST %s %s %s%s: iterate %d is %.3g from the oracle's" % (method, size, pre, " offset" * offset, n, err))
        assert got.count == want.count == n and len(got.hist) == len(want.hist)
        assert err <= 1e-11
        np.testing.assert_allclose(got.hist, want.hist, rtol=1e-8)
        worst = max(worst, err)
    return worst


def check_convergence(method, size, pre, offset=False):
    """Tolerance 1e-10: the count within max(3, 3 %) of the oracle's, the solution within 1e-8 of the dense solve."""
    got = solve(method, size, pre, 1e-10, 500, offset=offset)
    k = got.k if method == "bpcg1" else scale_of(size, pre) if method == "bpcg2" else 0.0
    want = reference(method, size, pre, k, 1e-10, 500)
    err, err_ref = sc.distance(got.x, exact_solution(size, pre)), sc.distance(want.x, exact_solution(size, pre))
    print("CONVERGED %s %s %s%s: %d iterations (oracle %d), %.3g from the dense solve (oracle %.3g)"
          % (method, size, pre, " offset" * offset, got.count, want.count, err, err_ref))
    assert want.count < 500 and err_ref <= 1e-9                 # the reference, as tests/test_saddle_cases_cpu.py holds it
    assert got.count < 500 and abs(got.count - want.count) <= max(3, int(0.03 * want.count))
    assert err <= 1e-8
    return got


# ---- (a), (b): every size, point Jacobi -----------------------------------------------------------------------------
@pytest.mark.parametrize("method", sc.METHODS)
@pytest.mark.parametrize("size", sc.SIZES, **ids)
def test_first_iterates_at_every_size(hip_engine, size, method):
    check_first_iterates(method, size, "point", (1, 2, 3))


@pytest.mark.parametrize("method", sc.METHODS)
@pytest.mark.parametrize("size", sc.SIZES, **ids)
def test_convergence_at_every_size(hip_engine, size, method):
    check_convergence(method, size, "point")


# ---- (c): block Jacobi ----------------------------------------------------------------------------------------------
BLOCK_CASES = ([(size, pre) for size in ((65, 64), (513, 511), (1025, 1)) for pre in ("runs2", "runs123", "runs2-uncovered")]
               + [((511, 255), "runs2")])


def test_the_block_cases_are_what_they_are_meant_to_be():
    counts = {(size, pre): len(blocks_of(pre, size[0])) for size, pre in BLOCK_CASES}
    assert [counts[(s, "runs2")] for s in ((65, 64), (513, 511), (1025, 1), (511, 255))] == [33, 257, 513, 256]
    assert [counts[(s, "runs2-uncovered")] for s in ((65, 64), (513, 511), (1025, 1))] == [32, 256, 512]
    for size, pre in BLOCK_CASES:
        blocks = blocks_of(pre, size[0])
        covered = sorted(d for b in blocks for d in b)
        assert covered == list(range(size[0] - (pre == "runs2-uncovered")))
        assert (len(blocks[-1]) == 1) == (pre == "runs2" and size[0] % 2 == 1) or pre == "runs123"


@pytest.mark.parametrize("method", sc.METHODS)
@pytest.mark.parametrize("size,pre", BLOCK_CASES, **ids)
def test_block_jacobi_with_blocks_no_grid_makes(hip_engine, size, pre, method):
    import hipla
    check_first_iterates(method, size, pre, (2,))
    got = check_convergence(method, size, pre)
    if pre == "runs2-uncovered":
        assert got.x[size[0] - 1] == 0.0                         # the dof in no block stays where it started
        Ad = hipla.SparseMatrix.from_scipy(sc.case(*size)[0])
        y = hipla.Vector(size[0])
        y.data = hipla.BlockJacobi(Ad, blocks_of(pre, size[0])) * hipla.Vector.from_numpy(np.ones(size[0]))
        assert y.numpy()[-1] == 0.0 and np.all(y.numpy()[:-1] != 0.0)     # exactly that dof is in no block


# ---- (d): the plan switches change no bit ---------------------------------------------------------------------------
SWITCHES = {"bpcg2": [("bpcg2_fold", 0), ("bpcg2_fold", 1), ("fuse_bjac", 0), ("fuse_bjac", 1), ("stream_loads", 1)],
            "bpcg1": [("bpcg1_fold", 0), ("bpcg1_fold", 1), ("stream_loads", 1)],
            "minres": [("minres_fold", 0), ("minres_fold", 1), ("minres_fuse", 0), ("minres_fuse", 1), ("stream_loads", 1)]}


DEFAULT_RUNS = {}        # (method, size, pre) -> the run with every switch at the library's default (read only)


@pytest.mark.parametrize("method,switch", [(m, s) for m in sc.METHODS for s in SWITCHES[m]],
                         ids=lambda v: "%s=%d" % v if isinstance(v, tuple) else v)
@pytest.mark.parametrize("pre", ["point", "runs2"])
@pytest.mark.parametrize("size", [(2, 1), (513, 511), (1537, 1025)], **ids)
def test_plan_switches_change_no_bit(hip_engine, size, pre, method, switch):
    """Three iterations under the switch against three at the defaults: history and solution with ==.

    [1537x1025-runs2-minres-minres_fuse=0] is the case that found the two forms of MINRES with a block Jacobi 2.3e-16
    apart: the fused M3 wrote the partials of <z_new, v_new> as one array [v0 .. v3, p0 .. p2], the stand-alone apply
    wrote [v0 .. v3] and M3 [0, 0, 0, 0, p0, p1, p2], and fixed_sum_1024 adds the two layouts in different orders.  Both
    forms write the first layout now (csrc/minres.hip: MK4Args::pfirst)."""
    if (method, size, pre) not in DEFAULT_RUNS:
        DEFAULT_RUNS[method, size, pre] = solve(method, size, pre, 0.0, 3)
    default = DEFAULT_RUNS[method, size, pre]
    assert default.count == 3
    with hip_engine.overrides(**{switch[0]: switch[1]}):       # (operands and plans are made under the switch)
        got = solve(method, size, pre, 0.0, 3)
    same = np.array_equal(got.x, default.x) and np.array_equal(got.hist, default.hist)
    print("SWITCH %s %s %s %s=%d: %s" % (method, size, pre, switch[0], switch[1], "same bits" if same else
                                          "%.3g apart, histories %.3g" % (sc.distance(got.x, default.x),
                                                                          np.max(np.abs(got.hist / default.hist - 1.0)))))
    np.testing.assert_array_equal(got.hist, default.hist)
    np.testing.assert_array_equal(got.x, default.x)


# ---- (e): solution and right-hand side off the 16-byte boundary ------------------------------------------------------
@pytest.mark.parametrize("method", sc.METHODS)
@pytest.mark.parametrize("size", [(3, 2), (513, 511), (1025, 1)], **ids)
def test_unaligned_solution_and_right_hand_side(hip_engine, size, method):
    check_first_iterates(method, size, "point", (3,), offset=True)
    got = check_convergence(method, size, "point", offset=True)
    aligned = solve(method, size, "point", 1e-10, 500)
    same = got.count == aligned.count and np.array_equal(got.x, aligned.x) and np.array_equal(got.hist, aligned.hist)
    print("OFFSET %s %s: %s the aligned run" % (method, size, "the bits of" if same else
                                                "%.3g from" % sc.distance(got.x, aligned.x)))


# ---- (f): the done word freezes the state -----------------------------------------------------------------------------
@pytest.mark.parametrize("method", sc.METHODS)
@pytest.mark.parametrize("size", [(1, 1), (513, 511)], **ids)
def test_the_done_word_freezes_the_state(hip_engine, size, method):
    outs = [solve(method, size, "point", 1e-10, 500, poll_every=every) for every in (1, 7, 1000)]
    assert outs[0].count < 500
    for got in outs[1:]:
        assert got.count == outs[0].count
        np.testing.assert_array_equal(got.hist, outs[0].hist)
        np.testing.assert_array_equal(got.x, outs[0].x)


# ---- (g): a zero right-hand side ------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", sc.METHODS)
def test_zero_right_hand_side_fused_and_protocol(hip_engine, method):
    """Both paths return the same values or raise the same exception type (the reference: BPCG v2 returns the bare zero
    vector at <w, d> == 0, :191-192; the textbook BPCG divides err / err0 at :118 and MINRES 1 / gamma at :73)."""
    import hipla
    from hipla import fused
    from bramble_pasciak_cg import bramble_pasciak_cg
    from minres import MinRes
    from solvers.bramblepasciak_new import BramblePasciakCG
    size = (3, 2)
    A, B, _, _, mass = sc.case(*size)
    loop = {"bpcg2": fused.Bpcg2Loop, "bpcg1": fused.Bpcg1Loop, "minres": fused.MinresLoop}[method]
    outcomes = {}
    for path in ("protocol", "fused"):
        Ad, Bd = hipla.SparseMatrix.from_scipy(A), hipla.SparseMatrix.from_scipy(B)
        preA, preS = hipla.JacobiPreconditioner(Ad), hipla.DiagonalMatrix(1.0 / mass)
        fv, gv = hipla.Vector(size[0]), hipla.Vector(size[1])
        sol = hipla.BlockVector([hipla.Vector.from_numpy(np.full(n, SENTINEL)) for n in size])
        if method == "bpcg1":
            sol[:] = 0.0                                             # (its start vector)
        loop.last_declined = "try_create was not called"
        fused.ENABLED = path == "fused"
        try:
            with contextlib.redirect_stdout(io.StringIO()):
                if method == "bpcg2":
                    ret = BramblePasciakCG(Form(Ad), Form(Bd), None, fv, gv, preA, preS, sol, tol=1e-10, maxsteps=20)
                    assert ret is sol                                # the bare vector, not (it, seconds)
                    ret = "the solution vector"
                elif method == "bpcg1":
                    ret = bramble_pasciak_cg(Ad, Bd, None, preA, preS, fv, gv, solution=sol, tolerance=1e-10,
                                             max_steps=20, print_rates=False)[1]
                else:
                    ret = MinRes(mat=hipla.BlockMatrix([[Ad, Bd.T], [Bd, None]]),
                                 pre=hipla.BlockMatrix([[preA, None], [None, preS]]), rhs=hipla.BlockVector([fv, gv]),
                                 sol=sol, maxsteps=20, tol=1e-10, printrates=False)[1]
            outcomes[path] = ("returned", ret)
        except Exception as exc:                                     # noqa: BLE001 (the type is what is compared)
            outcomes[path] = ("raised", type(exc))
        finally:
            fused.ENABLED = True
        if method != "minres":                                       # (MINRES divides before it reaches its loop)
            declined = loop.last_declined
            assert (declined is None) if path == "fused" else (declined is not None and "ENABLED" in declined), declined
        x = sol.numpy()
        assert np.isfinite(x).all() or not x.any()
        outcomes[path] += (x,)
        print("ZERO %s %s: %s" % (method, path, outcomes[path][:2]))
    assert outcomes["fused"][:2] == outcomes["protocol"][:2]
    np.testing.assert_array_equal(outcomes["fused"][2], outcomes["protocol"][2])
