"""The V-cycle with replicated coarse levels and MypreA's auxiliary-space term natively inside the partitioned BPCG v2
loop over the mailbox transport (csrc/p2p.h) with 2 and 3 processes on the one GPU, and the transport's vector
all-reduce with 2, 3 and 5 -- against numpy and the single-GPU solves with the same operators."""

import contextlib
import io
import os
import re
import subprocess
import sys
import tempfile

import numpy as np
import pytest

from conftest import ROOT
from staggered_grid import mac_stokes

pytestmark = pytest.mark.gpu

WORKER = os.path.join(ROOT, "tests", "mailbox_precond_worker.py")


def launch(world, mode, dim=0, n=0, pre="-", tol=1e-8, maxsteps=2000, timeout=600):
    tmp = tempfile.mkdtemp(prefix="nssmbx_")
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", OMP_NUM_THREADS="1", HSA_ENABLE_IPC_MODE_LEGACY="0")
    procs = [subprocess.Popen([sys.executable, WORKER, str(r), str(world), os.path.join(tmp, "rendezvous"), tmp, mode,
                               str(dim), str(n), pre, repr(tol), str(maxsteps)], env=env,
                              stdout=subprocess.PIPE, stderr=subprocess.STDOUT) for r in range(world)]
    outs = []
    for p in procs:
        try:
            o, _ = p.communicate(timeout=timeout)
        except subprocess.TimeoutExpired:
            for q in procs:
                q.kill()
            raise
        outs.append(o.decode(errors="replace"))
    for p, o in zip(procs, outs):
        assert p.returncode == 0, o[-3000:]
    return [np.load(os.path.join(tmp, "rank%d.npz" % r)) for r in range(world)]


class Form:
    def __init__(self, mat):
        self.mat, self.condense = mat, False


def single_solve(s, preA, tol, maxsteps):
    import hipla
    from solvers.bramblepasciak_new import BramblePasciakCG
    f, g = s.rhs(0)
    A, B = hipla.SparseMatrix.from_scipy(s.A), hipla.SparseMatrix.from_scipy(s.B)
    sol = hipla.BlockVector([hipla.Vector(s.n_u), hipla.Vector(s.n_p)])
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        it, _ = BramblePasciakCG(Form(A), Form(B), None, hipla.Vector.from_numpy(f), hipla.Vector.from_numpy(g), preA,
                                 hipla.DiagonalMatrix(1.0 / s.mass), sol, tol=tol, maxsteps=maxsteps)
    hist = np.array([float(m) for m in re.findall(r"it =\s+\d+\s+err =\s+(\S+)", out.getvalue())])
    return it, hist, sol[0].numpy()


@pytest.mark.parametrize("world", [2, 3, 5])
def test_vector_allreduce_adds_in_rank_order(world):
    """dst = the rank-ordered sum of the contributions inside the registered ranges, bit for bit on every rank, over
    three consecutive calls (both copies of the zone), for overlapping ranges, an empty range and full ranges."""
    from mailbox_precond_worker import contribution, vec_cases
    ranks = launch(world, "vec")
    for name, lo, hi in vec_cases(world):
        for call in range(3):
            key = "%s_%d" % (name, call)
            want = np.zeros_like(ranks[0][key])
            for q in range(world):
                want += contribution(q, call, lo[q], hi[q])[0]
            for d in ranks:
                np.testing.assert_array_equal(d[key], want)
                np.testing.assert_array_equal(d[key].view(np.int64), ranks[0][key].view(np.int64))
        for d in ranks:
            assert int(d["%s_timeout" % name]) == 0
            assert int(d["%s_seq" % name]) == 3


def check_common(ranks, it_s, hist_s, u_s, window, iters_band):
    for d in ranks:
        assert int(d["native"]) == 1 and int(d["mailbox"]) == 1 and str(d["declined"]) == "None"
        assert int(d["conv"]) == 1
        assert int(d["timeout"]) == 0 and int(d["timeout_after_profile"]) == 0
        np.testing.assert_array_equal(d["hist"], ranks[0]["hist"])            # same decision on every rank
        np.testing.assert_array_equal(d["channels"], ranks[0]["channels"])    # same channel numbering on every rank
        assert int(d["profile_n"]) == 12
    it = int(ranks[0]["it"])
    w = min(window, len(hist_s), len(ranks[0]["hist"]))
    np.testing.assert_allclose(ranks[0]["hist"][:w], hist_s[:w], rtol=1e-8)
    assert abs(it - it_s) <= iters_band(it_s)
    u = np.concatenate([d["u"] for d in ranks])
    assert np.linalg.norm(u - u_s) < 1e-5 * np.linalg.norm(u_s)


@pytest.mark.parametrize("world,dim,n", [(2, 3, 10), (3, 3, 12)])     # (3, 9): a single-level default hierarchy
@pytest.mark.parametrize("pre", ["amg", "amg+bjac"])
def test_amg_over_the_mailbox_matches_single_gpu(hip_engine, world, dim, n, pre):
    """pre="amg" / "amg+bjac" in the native loop over the mailbox transport: the V-cycle's halos on channel 0 (A's
    operand layout, t1's), its coarse all-reduce through the vector zone -- against the single-GPU solve with the same
    global hierarchy."""
    import hipla
    tol, maxsteps = 1e-8, 2000
    ranks = launch(world, "solve", dim, n, pre, tol, maxsteps)
    s = mac_stokes(dim, n, 0.01)
    A = hipla.SparseMatrix.from_scipy(s.A)
    V = hipla.SmoothedAggregationAMG(A)
    single = V if pre == "amg" else V + hipla.BlockJacobi(A, s.line_blocks(3))
    it_s, hist_s, u_s = single_solve(s, single, tol, maxsteps)
    for d in ranks:
        np.testing.assert_array_equal(d["channels"], [0, 0])                # t1 and the V-cycle share A's layout
    check_common(ranks, it_s, hist_s, u_s, 25, lambda it: max(3, int(0.03 * it)))


@pytest.mark.parametrize("world,dim,n", [(2, 3, 10), (3, 3, 9)])
def test_mypre_a_over_the_mailbox_matches_its_slab_twin(hip_engine, world, dim, n):
    """MypreA(GS=True) with the auxiliary-space term on slabs in the native loop over the mailbox transport: the native
    auxiliary apply equals the single-process transform V(L) transform^T, and the solve follows the single-GPU solve
    of the slab twin."""
    import hipla
    from test_distributed_cpu import slab_twin_of_mypre_a
    tol, maxsteps = 1e-8, 3000
    ranks = launch(world, "solve", dim, n, "mypre_a", tol, maxsteps)
    s = mac_stokes(dim, n, 0.01)
    twin, _, _, levels = slab_twin_of_mypre_a(s, world, s.line_blocks(3), coarse_size=40)
    st = s.auxiliary_space_stacked()
    V = hipla.SmoothedAggregationAMG(hipla.SparseMatrix.from_scipy(st["laplacian"]), coarse_size=40)
    aux = hipla.AuxiliarySpaceAMG(hipla.SparseMatrix.from_scipy(st["transform"]), [V])
    x = np.random.default_rng(9).standard_normal(s.n_u)
    y = hipla.Vector(s.n_u)
    y.data = aux * hipla.Vector.from_numpy(x)
    got = np.concatenate([d["aux_apply"] for d in ranks])
    for d in ranks:
        np.testing.assert_array_equal(d["aux_levels"], levels)
        # t1, transform.T's operand, transform's operand, t1 again (the residual), the nodal Laplacian's operand
        np.testing.assert_array_equal(d["channels"], [0, 1, 2, 0, 3])
    assert np.linalg.norm(got - y.numpy()) < 1e-12 * np.linalg.norm(y.numpy())
    it_s, hist_s, u_s = single_solve(s, twin, tol, maxsteps)
    check_common(ranks, it_s, hist_s, u_s, 20, lambda it: max(3, int(0.05 * it)))
