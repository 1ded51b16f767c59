"""The statically condensed Stokes solve on row-partitioned slabs (`DistributedStokes(condense=True)`), host logic on the
numpy checker engine with gloo process groups: the protocol solve on slabs against the single-rank condensed solve
(block Jacobi over S does not depend on the partition), the partitioned MypreA over S against its single-process slab
twin, and the combinations the native loop still declines."""

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
from oracle import krylov_ref as kr

WORKER = os.path.join(ROOT, "tests", "condensed_dist_worker.py")
AUX = dict(coarse_size=40)


def launch(world, mode, dim, n, pre, tol, maxsteps, timeout=600):
    """`world` fresh worker processes, each under its own time limit; the rest are killed at the first failure."""
    tmp = tempfile.mkdtemp(prefix="nsscond_")
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", OMP_NUM_THREADS="1", HSA_ENABLE_IPC_MODE_LEGACY="0")
    procs = [subprocess.Popen([sys.executable, WORKER, str(r), str(world), mode, os.path.join(tmp, "rendezvous"), tmp,
                               str(dim), str(n), pre, repr(tol), str(maxsteps)], env=env,
                              stdout=subprocess.PIPE, stderr=subprocess.STDOUT) for r in range(world)]
    try:
        for p in procs:
            out, _ = p.communicate(timeout=timeout)
            assert p.returncode == 0, out.decode(errors="replace")[-3000:]
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
                p.wait()
    return [np.load(os.path.join(tmp, "rank%d.npz" % r)) for r in range(world)]


def _history(text):
    return np.array([float(m) for m in re.findall(r"it =\s+\d+\s+err =\s+(\S+)", text)])


def single_rank_condensed(s, pre, tol, maxsteps):
    """The single-GPU condensed solve through the protocol: `CondensedForm` and block Jacobi over S with the facet
    blocks restricted to the coupling dofs."""
    import hipla
    from discretizations import AssembledForm, CondensedForm
    from solvers.bramblepasciak_new import BpcgSession
    from templates.NavierStokesSIMPLE_iterative import coupling_blocks
    blfA = CondensedForm(s)
    assert pre in ("bjac", "jacobi")
    preA = hipla.BlockJacobi(blfA.mat, coupling_blocks(s.facet_blocks(), blfA.interior)) if pre == "bjac" else blfA.jacobi()
    f, g = s.rhs(0)
    sol = hipla.BlockVector([hipla.Vector(s.n_u), hipla.Vector(s.n_p)])
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        ses = BpcgSession(blfA, AssembledForm(hipla.SparseMatrix.from_scipy(s.B)), None, hipla.Vector.from_numpy(f),
                          hipla.Vector.from_numpy(g), preA, hipla.DiagonalMatrix(1.0 / s.mass), sol=sol)
        it, _ = ses.protocol_loop(tol, maxsteps, True, True)
    return dict(it=it, hist=_history(out.getvalue()), k=ses.k, err0=ses.err0, u=sol[0].numpy(), p=sol[1].numpy())


@pytest.mark.parametrize("world,dim,n,pre", [(2, 3, 6, "bjac"), (3, 2, 12, "bjac"), (2, 2, 12, "bjac"), (3, 3, 6, "bjac"),
                                            (2, 3, 6, "jacobi")])
def test_condensed_on_slabs_matches_single_rank(numpy_engine, world, dim, n, pre):
    """Block Jacobi over S and (pre=None) point Jacobi on the coupling dofs do not depend on the partition."""
    from staggered_grid import mac_stokes
    # (tol 1e-6: below it the condensed solve's late iterations follow the rounding -- 3-D n = 6 stops at 93 on two slabs
    # and at 112 on one at 1e-8 with histories equal to 7e-12 up to iteration 56)
    tol, maxsteps = 1e-6, 3000
    ranks = launch(world, "cpu", dim, n, pre, tol, maxsteps)
    s = mac_stokes(dim, n, 0.01)
    ref = single_rank_condensed(s, pre, tol, maxsteps)
    interior = s.condense()["interior"]
    vel, prs = s.partition(world)
    # the 2-D condensed functional cancels after about a dozen iterations (tests/test_condensed_mypre_gpu.py)
    window = 12 if dim == 2 else 30
    for r, d in enumerate(ranks):
        assert list(d["slices"]) == [vel[r], vel[r + 1], prs[r], prs[r + 1]]
        # the coupling blocks leave exactly the owned interior dofs uncovered (no blocks: nothing is counted)
        assert int(d["n_uncovered"]) == (int(interior[vel[r]:vel[r + 1]].sum()) if pre == "bjac" else 0)
        assert abs(d["k"] - ref["k"]) < 1e-9 * ref["k"]
        assert abs(d["err0"] - ref["err0"]) < 1e-10 * ref["err0"]
        np.testing.assert_array_equal(d["hist"], ranks[0]["hist"])
        w = min(window, len(ref["hist"]), len(d["hist"]))
        np.testing.assert_allclose(d["hist"][:w], ref["hist"][:w], rtol=1e-8)
        assert abs(int(d["it"]) - ref["it"]) <= max(3, int(0.03 * ref["it"]))
    u = np.concatenate([d["u"] for d in ranks])
    p = np.concatenate([d["p"] for d in ranks])
    assert np.linalg.norm(u - ref["u"]) < 1e-5 * np.linalg.norm(ref["u"])
    p0, pr = p - p.mean(), ref["p"] - ref["p"].mean()
    assert np.linalg.norm(p0 - pr) < 1e-4 * np.linalg.norm(pr)


def slab_twin_of_condensed_mypre_a(s, world, residual="slab", **amg_options):
    """The single-process operator a `world`-way `DistributedStokes(pre="mypre_a", condense=True)` applies as preA:
    multicolour block Gauss-Seidel over the slab-block-diagonal part of S with the coupling facet blocks, the residual
    between the sweeps with that same slab-block-diagonal part (`residual="full"`: with the full S -- not symmetric),
    and one V-cycle of the stacked nodal Laplacian between `transform` and its transpose.  Returns (twin, parts)."""
    import hipla
    import scipy.sparse as sp
    from templates.NavierStokesSIMPLE_iterative import coupling_blocks
    parts = s.condense()
    S = parts["mat"]
    vel, _ = s.partition(world)
    bd = sp.block_diag([S[vel[r]:vel[r + 1], vel[r]:vel[r + 1]] for r in range(world)], format="csr")
    G = hipla.BlockGaussSeidel(hipla.SparseMatrix.from_scipy(bd), coupling_blocks(s.facet_blocks(), parts["interior"]))
    Sm = hipla.SparseMatrix.from_scipy(bd if residual == "slab" else S)
    st = s.auxiliary_space_stacked()
    V = hipla.SmoothedAggregationAMG(hipla.SparseMatrix.from_scipy(st["laplacian"]), **amg_options)
    aux = hipla.AuxiliarySpaceAMG(hipla.SparseMatrix.from_scipy(st["transform"]), [V])

    def apply(x):                                # templates/NavierStokesSIMPLE_iterative.py:377-381, over S
        xv, y = hipla.Vector.from_numpy(x), hipla.Vector(s.n_u)
        y[:] = 0.0
        G.Smooth(y, xv)
        res = hipla.Vector(s.n_u)
        res.data = xv - Sm * y
        y.data += aux * res
        G.SmoothBack(y, xv)
        return y.numpy()
    return apply, parts


def test_condensed_mypre_a_on_slabs_matches_its_slab_twin(numpy_engine):
    from staggered_grid import mac_stokes
    world, dim, n, tol, maxsteps = 2, 3, 6, 1e-8, 1000
    ranks = launch(world, "cpu", dim, n, "mypre_a", tol, maxsteps)
    s = mac_stokes(dim, n, 0.01)
    twin, parts = slab_twin_of_condensed_mypre_a(s, world, **AUX)
    H, HT, inner = parts["harmonic_extension"], parts["harmonic_extension_trans"], parts["inner_solve"]
    # one apply of the partitioned condensed step (scale 1.7) against the twin's
    x = np.random.default_rng(11).standard_normal(s.n_u)
    lifted = x + HT @ x
    y = 1.7 * twin(lifted)
    want = y + H @ y + inner @ lifted
    got = np.concatenate([d["step"] for d in ranks])
    assert np.linalg.norm(got - want) < 1e-12 * np.linalg.norm(want)
    for d in ranks:
        assert int(d["n_uncovered"]) == int(d["n_interior"]) > 0
        np.testing.assert_array_equal(d["hist"], ranks[0]["hist"])
    # the scale factor is positive (preA symmetric positive definite) and the oracle's Lanczos over the twin agrees with
    # it (another recurrence on A instead of the explicit product, both stopped at tol 1e-3: measured 2.6e-6 apart)
    k = float(ranks[0]["k"])
    k_twin = kr.scale_factor(kr.lanczos_ritz(s.A, twin, tol=1e-3))
    assert k > 0 and abs(k - k_twin) < 1e-5 * k_twin
    # the whole solve against the oracle's condensed BPCG v2 with the twin as preA, at the slabs' k
    f, g = s.rhs(0)
    condensed = {key: parts[key] for key in ("harmonic_extension", "harmonic_extension_trans", "inner_solve",
                                             "inner_matrix")}
    it_ref, u_ref, p_ref, hist_ref, err0 = kr.bpcg_v2(parts["mat"], s.B, twin, kr.diag_inverse(s.mass), f, g, k, tol=tol,
                                                      maxsteps=maxsteps, condensed=condensed)
    assert abs(float(ranks[0]["err0"]) - err0) < 1e-10 * err0
    assert 3 < it_ref < maxsteps - 1                                  # converged
    w = min(20, len(hist_ref), len(ranks[0]["hist"]))
    np.testing.assert_allclose(ranks[0]["hist"][:w], hist_ref[:w], rtol=1e-8)
    assert abs(int(ranks[0]["it"]) - it_ref) <= max(3, int(0.05 * it_ref))
    u = np.concatenate([d["u"] for d in ranks])
    assert np.linalg.norm(u - u_ref) < 1e-5 * np.linalg.norm(u_ref)


def test_residual_with_the_full_S_breaks_the_condensed_mypre_a(numpy_engine):
    """Why the slabs form MypreA's residual with the slab block of S: with the full S (sweeps and residual over different
    matrices) the preconditioner is not symmetric and the scale factor comes out negative on two slabs; with the slab
    block it is positive and close to the one-slab value."""
    from staggered_grid import mac_stokes
    s = mac_stokes(3, 6, 0.01)
    full, _ = slab_twin_of_condensed_mypre_a(s, 2, residual="full", **AUX)
    slab, _ = slab_twin_of_condensed_mypre_a(s, 2, **AUX)
    one, _ = slab_twin_of_condensed_mypre_a(s, 1, **AUX)
    k_full, k_slab, k_one = (kr.scale_factor(kr.lanczos_ritz(s.A, op, tol=1e-3)) for op in (full, slab, one))
    assert k_full < 0
    assert k_one > 0 and abs(k_slab - k_one) < 0.05 * k_one


class FakeComm:
    """A one-rank communicator without a process group (nothing to exchange or reduce)."""
    rank, size = 0, 1

    def gather_requests(self, mine, compute_for_rank):
        return [mine]

    def gather_objects(self, obj):
        return [obj]

    def allreduce_scalar(self, value):
        return float(value)

    def allreduce_sum(self, buf):
        pass

    def exchange(self, plan, sendbuf, ext):
        pass


def test_condensed_combinations_still_declined(numpy_engine, monkeypatch):
    """What stays unsupported is refused with a reason: operators not laid out for slabs, an AMG term with the
    condensed form on slabs, the V-cycle preconditioners, and MypreA over the mailbox transport."""
    import types

    import hipla
    from distributed import DistributedBpcg2
    from hipla import fused
    from staggered_grid import mac_stokes
    s = mac_stokes(2, 6, 0.01)
    parts = s.condense()
    ops = {key: hipla.SparseMatrix.from_scipy(parts[key]) for key in ("mat", "harmonic_extension",
                                                                      "harmonic_extension_trans", "inner_solve")}
    condensed = dict(HT=ops["harmonic_extension_trans"], H=ops["harmonic_extension"], inner=ops["inner_solve"],
                     S=ops["mat"])
    A, B = hipla.SparseMatrix.from_scipy(s.A), hipla.SparseMatrix.from_scipy(s.B)
    BT = B.CreateTranspose()
    vecs = {name: hipla.Vector(s.n_u) for name in ("u0", "d0", "w0", "s0", "z0", "q", "t0", "t1", "t2", "t4")}
    vecs.update({name: hipla.Vector(s.n_p) for name in ("u1", "d1", "w1", "s1", "t3")})
    preM = hipla.DiagonalMatrix(1.0 / s.mass)
    jac = hipla.DiagonalMatrix(np.ones(s.n_u))
    monkeypatch.setattr(fused, "_hip", lambda eng: True)
    Loop = fused.Bpcg2Loop
    assert Loop.try_create(A, B, BT, jac, 1.0, preM, vecs, distributed=True, condensed=condensed) is None
    assert Loop.last_declined == "condensed form on a partitioned run"
    slab = dict(condensed, slab=True)
    amg = hipla.SmoothedAggregationAMG(A, coarse_size=40)
    assert Loop.try_create(A, B, BT, amg, 1.0, preM, vecs, distributed=True, condensed=slab) is None
    assert Loop.last_declined == "condensed form on a partitioned run with an AMG term"
    aux = types.SimpleNamespace()
    assert Loop.try_create(A, B, BT, None, 1.0, preM, vecs, distributed=True, condensed=slab, dist_aux=aux) is None
    assert "auxiliary-space term only inside the multiplicative MypreA" in Loop.last_declined
    narrow = dict(slab, H=hipla.SparseMatrix.from_scipy(parts["harmonic_extension"][:, : s.n_u - 1]))
    assert Loop.try_create(A, B, BT, jac, 1.0, preM, vecs, distributed=True, condensed=narrow) is None
    assert Loop.last_declined == "condensed operators are not n_u x n_u SparseMatrix"
    monkeypatch.undo()
    f, g = s.rhs(0)
    for pre in ("amg", "amg+bjac"):
        with pytest.raises(ValueError, match="condense=True takes pre"):
            DistributedBpcg2(s, f, g, s.facet_blocks(), None, comm=types.SimpleNamespace(rank=0, size=1), pre=pre,
                             condense=True)
    with pytest.raises(ValueError, match="not positive"):
        DistributedBpcg2(s, f, g, s.facet_blocks(), None, comm=FakeComm(), pre="bjac", condense=True, k=-0.5)
    with pytest.raises(ValueError, match="mailbox"):
        DistributedBpcg2(s, f, g, s.facet_blocks(), None, comm=types.SimpleNamespace(rank=0, size=1), pre="mypre_a",
                         condense=True, transport="mailbox")


def test_native_loop_declines_off_the_hip_engine(numpy_engine):
    """DistributedBpcg2(condense=True) tells why there is no native loop (here: the checker engine)."""
    import torch.distributed as dist
    from distributed import DistributedBpcg2, TorchComm
    from staggered_grid import mac_stokes
    s = mac_stokes(2, 6, 0.01)
    f, g = s.rhs(0)
    tmp = tempfile.mkdtemp(prefix="nsscond1_")
    dist.init_process_group("gloo", init_method="file://" + os.path.join(tmp, "rdv"), rank=0, world_size=1)
    try:
        import hipla
        comm = TorchComm(dist, hipla.get_engine())
        made = []
        orig = DistributedBpcg2._attach

        def spy(self, vecs):
            made.append(self)
            return orig(self, vecs)
        DistributedBpcg2._attach = spy
        try:
            with pytest.raises(RuntimeError, match="not the HIP engine"):
                DistributedBpcg2(s, f, g, s.facet_blocks(), dist, comm=comm, pre="bjac", condense=True, k=1.5)
        finally:
            DistributedBpcg2._attach = orig
        assert made and made[0].declined == "not the HIP engine"
        assert made[0].k == 1.5 and made[0].ops.n_uncovered > 0
    finally:
        dist.destroy_process_group()
