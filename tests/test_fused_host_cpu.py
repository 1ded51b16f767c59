"""Host side of the fused loops on the numpy checker engine: which preconditioners each loop takes (the decoder
table), the chunked driver's windows and result conventions, and the mailbox timeout check of the partitioned MINRES
and BPCG v1 runs.  Nothing here touches a device: the loops' enqueue / poll are stand-ins."""
import pytest
import torch

from staggered_grid import mac_stokes


@pytest.fixture
def shapes(numpy_engine):
    """name -> preconditioner of every operator shape the decoder sorts, and the parts it is built from."""
    import hipla
    s = mac_stokes(2, 6, 0.01)
    A = hipla.SparseMatrix.from_scipy(s.A)
    blocks = s.line_blocks(3)
    D, BJ, GS = hipla.DiagonalMatrix(1.0 / s.A.diagonal()), hipla.BlockJacobi(A, blocks), hipla.BlockGaussSeidel(A, blocks)
    AMG = hipla.SmoothedAggregationAMG(A, coarse_size=40)
    GSM = hipla.BlockGaussSeidel(A, blocks, middle=AMG)
    ops = {"diag": D, "2 diag": 2.0 * D, "bjac": BJ, "2 bjac": 2.0 * BJ, "gs": GS, "gs+middle": GSM, "amg": AMG,
           "amg+diag": AMG + D, "amg+bjac": AMG + BJ, "amg+gs": AMG + GS, "2 amg": 2.0 * AMG, "amg-diag": AMG - D,
           "matrix": A}
    return s, A, ops, dict(D=D, BJ=BJ, GS=GS, AMG=AMG, GSM=GSM)


# (scale, diag, bjac, amg) of the decoder, then what each loop takes: "=" the decoder's record, "-" declined
DECODED = {
    "diag": ((1.0, "D", None, None), "=", "=", "=", "=", "="),
    "2 diag": ((2.0, "D", None, None), "=", "=", "-", "=", "="),
    "bjac": ((1.0, None, "BJ", None), "=", "=", "=", "=", "="),
    "2 bjac": ((2.0, None, "BJ", None), "-", "=", "-", "-", "="),
    "gs": ((1.0, None, "GS", None), "=", "=", "=", "=", "="),
    "gs+middle": ((1.0, None, "GSM", "AMG"), "-", "-", "-", "-", "-"),      # the multiplicative MypreA
    "amg": ((1.0, None, None, "AMG"), "=", "=", "=", "-", "-"),
    "amg+diag": ((1.0, "D", None, "AMG"), "=", "=", "-", "-", "-"),
    "amg+bjac": ((1.0, None, "BJ", "AMG"), "=", "=", "-", "-", "-"),
    "amg+gs": (None, "-", "-", "-", "-", "-"),
    "2 amg": ((2.0, None, None, "AMG"), "-", "-", "-", "-", "-"),
    "amg-diag": (None, "-", "-", "-", "-", "-"),
    "matrix": (None, "-", "-", "-", "-", "-"),
}


def test_preconditioner_decoder_table(shapes, monkeypatch):
    """native_velocity_pre (BPCG v2, Lanczos) and what MINRES, BPCG v1, CG and the partitioned MINRES / BPCG v1 take
    of it -- the first three through their own try_create, past the engine check, with a constructor that records."""
    import hipla
    from hipla import fused
    s, A, ops, parts = shapes
    monkeypatch.setattr(fused, "_hip", lambda eng: True)
    made = []

    def recording(base):
        class Probe(base):
            def __init__(self, eng, *args):
                made.append(args)
        return Probe

    B = hipla.SparseMatrix.from_scipy(s.B)
    BT = B.CreateTranspose()
    preS = 3.0 * hipla.DiagonalMatrix(1.0 / s.mass)
    blockvec = lambda: hipla.BlockVector([hipla.Vector(s.n_u), hipla.Vector(s.n_p)])      # noqa: E731

    def minres(op):
        K, C = hipla.BlockMatrix([[A, BT], [B, None]]), hipla.BlockMatrix([[op, None], [None, preS]])
        loop = recording(fused.MinresLoop).try_create(K, C, blockvec(), [blockvec() for _ in range(3)],
                                                      [blockvec() for _ in range(3)], [blockvec() for _ in range(2)],
                                                      blockvec())
        return loop, (made[-1][3], made[-1][4]) if loop is not None else None

    def bpcg1(op):
        vecs = {name: blockvec() for name in ("x", "r", "d", "a", "t1", "t2")}
        loop = recording(fused.Bpcg1Loop).try_create(A, B, None, op, preS, 1.0, vecs)
        return loop, (made[-1][2], made[-1][3]) if loop is not None else None

    def cg(op):
        loop = recording(fused.CgLoop).try_create(A, op)
        return loop, (made[-1][1], None) if loop is not None else None

    def named(p):
        if p is None:
            return None
        name = {id(v): k for k, v in parts.items()}
        return (p.scale,) + tuple(None if x is None else name[id(x)] for x in (p.diag, p.bjac, p.amg))

    for label, op in ops.items():
        want, *takes = DECODED[label]
        got = fused.native_velocity_pre(op)
        assert named(got) == want, label
        assert got is None or got.multiplicative == (label == "gs+middle")
        for kind, take in zip(("minres", "bpcg1", "cg"), takes):
            loop, recorded = {"minres": minres, "bpcg1": bpcg1, "cg": cg}[kind](op)
            Loop = type(loop) if loop is not None else None
            if take == "-":
                assert loop is None, (label, kind)
                continue
            assert loop is not None and Loop.last_declined is None, (label, kind)
            assert named(recorded[0]) == want, (label, kind)
            if recorded[1] is not None:                                   # preS: the scaled diagonal, as it is
                assert recorded[1].scale == 3.0 and recorded[1].diag is preS.mat
        for kind, take in zip(("partitioned minres", "partitioned bpcg1"), takes[3:]):
            assert named(fused.pre_for(kind, op)) == (None if take == "-" else want), (label, kind)
    assert cg(None)[1][0] is fused.NO_PRE
    # preM / preS: a (scaled) diagonal only
    assert named(fused.native_diag(ops["2 diag"])) == (2.0, "D", None, None)
    assert all(fused.native_diag(ops[k]) is None for k in ("bjac", "amg", "amg+diag", "matrix"))
    assert fused.native_diag(None) is None


# ---- the chunked driver -------------------------------------------------------------------------------------------
class FakeEngine:
    """What the loops' `run` / `solve` need of an engine besides their enqueue / poll: host buffers."""
    torch, device, stream = torch, "cpu", None

    def zeros(self, n):
        return torch.zeros(n, dtype=torch.float64)

    def upload(self, arr, buf):
        buf[: arr.size].copy_(torch.from_numpy(arr))

    def to_host(self, buf):
        return buf.numpy()

    def fill(self, x, v):
        pass

    def copy(self, a, b):
        pass

    def dot(self, a, b):
        return 4.0


class Stub:
    """Library stand-in: the loops only name its workspace queries (fit_partials is stubbed)."""

    def __getattr__(self, name):
        return None


def fake(base, stop_at, first=0):
    """A `base` loop whose enqueue records its windows and whose poll reports a stop once iteration `stop_at` ran
    (None: never).  `first`: the loop's first iteration index (MINRES counts from 1)."""
    from hipla import fused

    class Fake(base):
        def __init__(self):
            self.eng, self.lib, self.partials = FakeEngine(), Stub(), []
            self.state = {fused.Bpcg2Loop: fused.Bpcg2State, fused.MinresLoop: fused.MinresState,
                          fused.Bpcg1Loop: fused.Bpcg1State, fused.CgLoop: fused.CgState}[base]()
            self.scal, self.ctrl = self.eng.zeros(64), torch.zeros(8, dtype=torch.int32)
            self.pa, self.work = fused.NO_PRE, {k: None for k in ("r", "z", "p", "q")}
            self.windows, self.ran = [], first - 1

        def enqueue(self, a, b):
            assert a == self.ran + 1
            self.windows.append((a, b))
            self.ran = b - 1

        def poll(self):
            stop = stop_at is not None and self.ran >= stop_at
            return (stop, stop_at if stop else 0) + {fused.Bpcg2Loop: (self.ran,), fused.MinresLoop: (1,)}.get(base, ())
    return Fake()


@pytest.fixture
def no_partials(monkeypatch):
    from hipla import fused
    monkeypatch.setattr(fused, "fit_partials", lambda eng, st, workspace, mats, partials=None: partials)


def windows(begin, end, every):
    return [(a, min(end, a + every)) for a in range(begin, end, every)]


@pytest.mark.parametrize("every", [1, 7, 45])
def test_chunked_driver_windows(every):
    """`run_chunked` enqueues [begin, end) in windows of `poll_every`, polls after each and stops at the first poll
    that says so; the last poll result is what it returns."""
    from hipla.fused import run_chunked
    for stop_at in (None, 0, 12, 39):
        got, polls = [], []

        def poll():
            polls.append(got[-1][1])
            return (stop_at is not None and got[-1][1] > stop_at, got[-1][1])

        out = run_chunked(lambda a, b: got.append((a, b)), poll, 0, 40, every)
        full = windows(0, 40, every)
        upto = len(full) if stop_at is None else next(i for i, w in enumerate(full) if w[1] > stop_at) + 1
        assert got == full[:upto] and polls == [w[1] for w in full[:upto]]
        assert out == (stop_at is not None, full[upto - 1][1])


@pytest.mark.parametrize("every", [1, 7, 45])
def test_loop_result_conventions(no_partials, every):
    """What each loop returns from the driver's last poll: BPCG v2 the stopping iteration or maxsteps - 1, MINRES
    errors up to k_stop (k counts from 1 to maxsteps + 1), BPCG v1 and CG the count it + 1 (or maxsteps)."""
    from hipla import fused
    maxsteps = 40
    for stop_at in (None, 5, 39):
        done = stop_at is not None
        loop = fake(fused.Bpcg2Loop, stop_at)
        it, hist, converged = loop.run(1.0, 1.0, 1e-8, False, maxsteps, poll_every=every)
        assert (it, converged, len(hist)) == ((stop_at, True, stop_at + 1) if done else (maxsteps - 1, False, maxsteps))
        assert loop.windows == windows(0, maxsteps, every)[:len(loop.windows)] and loop.windows[-1][1] > it

        k_stop = stop_at + 1 if done else None            # MINRES: iterations k = 1 .. maxsteps
        loop = fake(fused.MinresLoop, k_stop, first=1)
        errors, hit_rel = loop.run(1.0, 1e-8, maxsteps, poll_every=every)
        assert len(errors) == (k_stop + 1 if done else maxsteps + 1) and hit_rel == done
        assert loop.windows == windows(1, maxsteps + 1, every)[:len(loop.windows)]

        loop = fake(fused.Bpcg1Loop, stop_at)
        errors, converged = loop.run(1.0, 1.0, 1e-8, maxsteps, poll_every=every)
        assert (len(errors), converged) == ((stop_at + 1, True) if done else (maxsteps, False))
        assert loop.windows == windows(0, maxsteps, every)[:len(loop.windows)]

        loop = fake(fused.CgLoop, stop_at)
        count, errors = loop.solve(None, torch.zeros(1), 1e-8, maxsteps, poll_every=every)
        assert (count, len(errors)) == ((stop_at + 1, stop_at + 2) if done else (maxsteps, maxsteps + 1))
        assert errors[0] == 2.0 and loop.windows == windows(0, maxsteps, every)[:len(loop.windows)]


class FakeTransport:
    """A mailbox transport that reports a timeout from its `after`-th check on."""

    def __init__(self, after):
        self.after, self.checks = after, 0

    def timed_out(self):
        self.checks += 1
        return self.checks >= self.after

    def close(self):
        pass


def test_partitioned_runs_raise_on_a_mailbox_timeout(no_partials):
    """The partitioned MINRES and BPCG v1 runs check their mailbox transport after every poll: a peer that did not
    arrive ends the run with the error BPCG v2's in-kernel check raises, instead of a wrong solution."""
    import distributed
    from hipla import fused

    class Minres(distributed.DistributedMinres):
        def _iterate(self, k_begin, k_end):
            self.loop.enqueue(k_begin, k_end)

    class Bpcg1(distributed.Bpcg1DistLoop):
        def enqueue(self, it_begin, it_end):
            self.loop.enqueue(it_begin, it_end)

    for after in (1, 3, None):
        mr = Minres.__new__(Minres)
        mr.loop, mr.gamma, mr.u = fake(fused.MinresLoop, None, first=1), 1.0, "u"
        bp = Bpcg1.__new__(Bpcg1)
        bp.loop = fake(fused.Bpcg1Loop, None)
        runs = ((mr, lambda: mr.solve(1e-8, 100, poll_every=10)), (bp, lambda: bp.run(1.0, 1.0, 1e-8, 100, poll_every=10)))
        for run, call in runs:
            run.mailbox = FakeTransport(after or 1000)
            if after is None:
                call()
                assert run.mailbox.checks == 10 and len(run.loop.windows) == 10
            else:
                with pytest.raises(RuntimeError, match="a peer did not arrive within the timeout"):
                    call()
                assert run.mailbox.checks == after and len(run.loop.windows) == after
            run.mailbox = None
