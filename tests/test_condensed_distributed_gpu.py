"""The statically condensed Stokes solve on row-partitioned slabs in the NATIVE compact loop: on a 1-rank RCCL
communicator against the single-GPU fused condensed loop, over the mailbox transport with 2 and 3 processes on the one
GPU against the protocol solve of the same partition, and the mailbox bookkeeping with an empty halo on a channel."""

import contextlib
import io
import re

import numpy as np
import pytest

from staggered_grid import mac_stokes
from test_condensed_distributed_cpu import launch

pytestmark = pytest.mark.gpu

AUX = dict(coarse_size=300)


def _history(text):
    return np.array([float(m) for m in re.findall(r"it =\s+\d+\s+err =\s+(\S+)", text)])


def single_gpu_condensed(s, pre, k=None):
    """BpcgSession on the single-GPU `CondensedForm` with block Jacobi over S, or the multiplicative MypreA over S
    (sweeps, residual with S, the auxiliary-space V-cycle on the stacked nodal Laplacian)."""
    import hipla
    from discretizations import AssembledForm, CondensedForm
    from solvers.bramblepasciak_new import BpcgSession
    from templates.NavierStokesSIMPLE_iterative import coupling_blocks
    blfA = CondensedForm(s)
    blocks = coupling_blocks(s.facet_blocks(), blfA.interior)
    if pre == "bjac":
        preA = hipla.BlockJacobi(blfA.mat, blocks)
    else:
        st = s.auxiliary_space_stacked()
        V = hipla.SmoothedAggregationAMG(hipla.SparseMatrix.from_scipy(st["laplacian"]), **AUX)
        preA = hipla.BlockGaussSeidel(blfA.mat, blocks,
                                      middle=hipla.AuxiliarySpaceAMG(hipla.SparseMatrix.from_scipy(st["transform"]), [V]))
    f, g = s.rhs(0)
    sol = hipla.BlockVector([hipla.Vector(s.n_u), hipla.Vector(s.n_p)])
    with contextlib.redirect_stdout(io.StringIO()):
        ses = BpcgSession(blfA, AssembledForm(hipla.SparseMatrix.from_scipy(s.B)), None, hipla.Vector.from_numpy(f),
                          hipla.Vector.from_numpy(g), preA, hipla.DiagonalMatrix(1.0 / s.mass), sol=sol, k=k)
    return ses, sol


@pytest.mark.parametrize("pre", ["bjac", "mypre_a"])
def test_native_condensed_compact_single_rank(hip_engine, tmp_path, pre):
    import torch.distributed as dist
    from distributed import DistributedBpcg2
    from rccl_comm import RcclComm
    s = mac_stokes(3, 12, 0.01)
    f, g = s.rhs(0)
    tol, maxsteps = (1e-6, 3000) if pre == "bjac" else (1e-8, 2000)
    ses0, _ = single_gpu_condensed(s, pre)
    assert ses0.fused is not None, ses0.fused_declined
    from hipla import eigen
    eigen.NATIVE = False                  # the same k through the protocol recurrence (the one the slabs run)
    try:
        ses_p, _ = single_gpu_condensed(s, pre)
    finally:
        eigen.NATIVE = True
    dist.init_process_group("gloo", init_method="file://" + str(tmp_path / "rdv"), rank=0, world_size=1)
    try:
        comm = RcclComm(dist, hip_engine)
        free = DistributedBpcg2(s, f, g, s.facet_blocks(), dist, hip_engine, comm=comm, pre=pre, condense=True,
                                aux_options=AUX if pre == "mypre_a" else None)
        assert free.native is not None and free.compact and free.declined is None
        # the two scale factors, each from its own Lanczos.  Block Jacobi: to 1e-10 against the single-GPU device and
        # protocol recurrences (measured 1e-15).  MypreA: its V-cycle rounds differently on slabs (DistributedAMG) and on
        # one GPU (the joint auxiliary cycle), and a Lanczos stopped at tol 1e-3 with orthogonality lost magnifies that --
        # measured 1.2e-5 against the device recurrence and 1.6e-5 against the single-GPU PROTOCOL recurrence, which differ
        # from each other by 2.7e-5: to 1e-4
        tol_k = 1e-10 if pre == "bjac" else 1e-4
        assert abs(free.k - ses_p.k) < tol_k * ses_p.k
        assert abs(free.k - ses0.k) < tol_k * ses0.k
        assert free.ops.n_uncovered == int(free.ops.form.interior.sum()) > 0
        if pre == "mypre_a":          # the slab sweep keeps the uncovered (interior) dofs as trailing columns
            assert free.ops.gs.layout == "colour-major" and free.ops.gs.n_uncovered == free.ops.n_uncovered
        free.release()
        # the loops at the same k
        run = DistributedBpcg2(s, f, g, s.facet_blocks(), dist, hip_engine, comm=comm, pre=pre, condense=True, k=ses0.k,
                               aux_options=AUX if pre == "mypre_a" else None)
        it, conv = run.solve(tol=tol, maxsteps=maxsteps, poll_every=16)
        hist = run.history(it)
        ses, sol = single_gpu_condensed(s, pre, k=ses0.k)
        from hipla import fused
        runs, orig_run = [], fused.Bpcg2Loop.run
        fused.Bpcg2Loop.run = lambda self, *a, **k: (runs.append(1), orig_run(self, *a, **k))[1]
        try:
            ses.first_direction()
            it_s, hist_s, conv_s = ses.fused.run(ses.wdn, ses.err0, tol, True, maxsteps)
        finally:
            fused.Bpcg2Loop.run = orig_run
        assert runs == [1]                                                 # the single-GPU fused condensed loop
        hist_s = np.asarray(hist_s)
        if pre == "bjac":
            assert conv and conv_s and it == it_s
            np.testing.assert_allclose(hist, hist_s, rtol=1e-12)
            assert np.linalg.norm(run.sol[0].numpy() - sol[0].numpy()) < 1e-10 * np.linalg.norm(sol[0].numpy())
        else:                         # the contract of test_native_partitioned_mypre_a_single_rank
            assert conv and conv_s and it < maxsteps - 1
            w = min(20, len(hist), len(hist_s))
            np.testing.assert_allclose(hist[:w], hist_s[:w], rtol=1e-8)
            assert abs(it - it_s) <= max(3, int(0.05 * it_s))
            assert np.linalg.norm(run.sol[0].numpy() - sol[0].numpy()) < 1e-5 * np.linalg.norm(sol[0].numpy())
        run.release()
        comm.close()
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("world,pre", [(2, "bjac"), (2, "bgs"), (3, "bjac"), (3, "bgs")])
def test_native_condensed_over_the_mailbox(hip_engine, world, pre):
    """The native condensed compact loop over the mailbox transport (t1, the lift and the extension on channels 0, 1,
    2) against the protocol solve of the same partition at the same k."""
    dim, n, tol, maxsteps = 2, 16, 1e-6, 3000
    ranks = launch(world, "mailbox", dim, n, pre, tol, maxsteps, timeout=900)
    for d in ranks:
        assert int(d["timeout"]) == 0
        np.testing.assert_array_equal(d["hist"], ranks[0]["hist"])
        ref = d["ref_hist"]
        w = min(12, len(ref), len(d["hist"]))
        np.testing.assert_allclose(d["hist"][:w], ref[:w], rtol=1e-8)
        assert abs(int(d["it"]) - int(d["ref_it"])) <= max(3, int(0.03 * int(d["ref_it"])))
    s = mac_stokes(dim, n, 0.01)
    sol = single_gpu_solution(s)
    u = np.concatenate([d["u"] for d in ranks])
    assert np.linalg.norm(u - sol) < 1e-4 * np.linalg.norm(sol)


def single_gpu_solution(s):
    """The single-GPU condensed solve with block Jacobi over S, to tol 1e-8: the reference for stitched solutions."""
    ses, sol = single_gpu_condensed(s, "bjac")
    ses.first_direction()
    ses.fused.run(ses.wdn, ses.err0, 1e-8, True, 3000)
    return sol[0].numpy()


def test_mailbox_bookkeeping_with_an_empty_halo(hip_engine):
    """Three ranks; on channel 1 rank 2 has an empty halo.  After the exchanges and BEFORE any all-reduce every rank
    reports the same sequence number and channel counts; only then the all-reduces run, with the right values."""
    ranks = launch(3, "p2p", 2, 12, "none", 0.0, 0, timeout=300)
    early = [(int(d["seq_early"]), list(d["counts_early"])) for d in ranks]
    assert all(int(d["agreed"]) == 1 for d in ranks), early
    assert early == [(3, [0, 3])] * 3
    assert [int(d["seq"]) for d in ranks] == [5, 5, 5] and [list(d["counts"]) for d in ranks] == [[1, 4]] * 3
    for r, d in enumerate(ranks):
        assert int(d["timeout"]) == 0
        assert float(d["ghost"]) == {0: 20.0, 1: 10.0, 2: -1.0}[r]     # ranks 0 and 1 swap buf[0] = 10 (rank + 1)
        np.testing.assert_array_equal(d["allreduce"], [6.0 + 300.0 * rep for rep in range(4)])
