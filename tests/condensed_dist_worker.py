"""Worker of the condensed row-partitioned tests (tests/test_condensed_distributed_*.py): one rank of a gloo process group.

argv: rank world mode init_file out_dir dim n pre tol maxsteps
mode "cpu":     numpy checker engine -- the condensed saddle system on slabs through the operator protocol
                (`DistributedStokes(condense=True)`, the reference's `BpcgSession` on `ops.form`), plus one apply of the
                partitioned condensed preconditioner step.
mode "mailbox": HIP engine, every rank on the one visible GPU -- the native condensed compact loop over the mailbox
                transport against the protocol solve of the same partition (same k).
mode "p2p":     HIP engine -- mailbox bookkeeping with a hand-built layout on which one rank has an empty halo.
Writes rank<r>.npz into out_dir."""

import contextlib
import io
import os
import re
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "navier-stokes-solver_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

AUX = dict(coarse_size=40)


def _history(text):
    return np.array([float(m) for m in re.findall(r"it =\s+\d+\s+err =\s+(\S+)", text)])


def protocol_solve(ops, f, g, tol, maxsteps, k=None):
    import hipla
    from distributed import Form
    from solvers.bramblepasciak_new import BpcgSession
    us, ps = ops.local_slices()
    sol = hipla.BlockVector([hipla.Vector(ops.n_u, engine=ops.engine), hipla.Vector(ops.n_p, engine=ops.engine)])
    sink = io.StringIO()
    with contextlib.redirect_stdout(sink):
        ses = BpcgSession(ops.form, Form(ops.B), None, hipla.Vector.from_numpy(f[us], engine=ops.engine),
                          hipla.Vector.from_numpy(g[ps], engine=ops.engine), ops.preA, ops.preM, sol=sol,
                          inner=ops.inner, k=k)
        it, _ = ses.protocol_loop(tol, maxsteps, True, True)
    return dict(hist=_history(sink.getvalue()), it=it, k=ses.k, err0=ses.err0, u=sol[0].numpy(), p=sol[1].numpy())


def run_p2p(rank, world, comm, eng, res):
    """Channel 0: A's operand of a real slab partition (every rank has a neighbour); channel 1: a hand-built layout in
    which ranks 0 and 1 swap one entry and rank 2 has an EMPTY halo.  Exchanges first, then the bookkeeping, then
    all-reduces."""
    import ctypes as C

    import torch
    from distributed import DistributedStokes, MailboxTransport
    from hipla.fused import HaloStruct
    from staggered_grid import mac_stokes
    sysm = mac_stokes(2, 12, 0.01)
    ops = DistributedStokes(sysm, None, comm, eng)
    probe = ops.A.operand()
    h0 = ops.A.native_halo(probe, (0, 0))
    n_own = 4
    buf = torch.zeros(n_own + 1, dtype=torch.float64, device=eng.device)
    buf[:n_own] = torch.arange(n_own, dtype=torch.float64, device=eng.device) + 10.0 * (rank + 1)
    h1 = HaloStruct()
    keep = []

    def table(name, vals, dt):
        arr = np.ascontiguousarray(vals, dtype=dt)
        keep.append(arr)
        setattr(h1, name, arr.ctypes.data if arr.size else None)

    peer = {0: 1, 1: 0}.get(rank)
    if peer is None:
        for name in ("h_send_peer", "h_send_off", "h_send_cnt", "h_recv_peer", "h_recv_off", "h_recv_cnt"):
            setattr(h1, name, None)
        h1.n_send = h1.n_recv = 0
    else:
        table("h_send_peer", [peer], np.int32), table("h_send_off", [0], np.int64), table("h_send_cnt", [1], np.int64)
        table("h_recv_peer", [peer], np.int32), table("h_recv_off", [n_own], np.int64), table("h_recv_cnt", [1], np.int64)
        h1.n_send = h1.n_recv = 1
    h1.n_pack, h1.direct, h1.int_begin, h1.int_end = 0, 1, 0, 0
    h1.send_idx = h1.sendbuf = None
    h1.ext = buf.data_ptr()
    mb = MailboxTransport(comm, eng, [(h0, ops.n_u), (h1, n_own)])
    # only channel 1 first: ranks 0 and 1 wait for each other alone, rank 2 has nothing to wait for -- whatever the
    # bookkeeping, nothing here can spin on a rank that is out of step
    for _ in range(3):
        mb.exchange(1)
    torch.cuda.synchronize()
    seq, counts = mb.counters()
    res["seq_early"], res["counts_early"] = seq, np.array(counts)
    # every rank must agree on the bookkeeping before anything else goes through the mailboxes (an exchange involving
    # every rank, or an all-reduce, would spin until the timeout on a rank that is out of step)
    agreed = comm.gather_objects((seq, tuple(counts)))
    res["agreed"] = int(all(a == agreed[0] for a in agreed))
    if res["agreed"]:
        mb.exchange(0)
        mb.exchange(1)
        torch.cuda.synchronize()
        seq, counts = mb.counters()
        res["seq"], res["counts"] = seq, np.array(counts)
        res["ghost"] = float(buf[n_own].cpu()) if peer is not None else -1.0
        vals = []
        for rep in range(4):
            src = torch.tensor([1.0 + rank + 100.0 * rep], dtype=torch.float64, device=eng.device)
            dst = torch.zeros(1, dtype=torch.float64, device=eng.device)
            mb.allreduce(src, dst)
            vals.append(float(dst.cpu()[0]))
        res["allreduce"] = np.array(vals)
    res["timeout"] = int(mb.timed_out())
    mb.close()
    del keep, C


def run(rank, world, mode, init_file, out_dir, dim, n, pre, tol, maxsteps):
    import torch
    import torch.distributed as dist
    dist.init_process_group("gloo", init_method="file://" + init_file, rank=rank, world_size=world)
    import hipla
    if mode == "cpu":
        from oracle.numpy_engine import NumpyEngine
        hipla.set_engine(NumpyEngine())
    else:
        torch.cuda.set_device(0)
        hipla.set_engine(None)
    eng = hipla.get_engine()
    from distributed import DistributedBpcg2, DistributedStokes, TorchComm
    from solvers.bramblepasciak_new import harmonic_extension
    from staggered_grid import mac_stokes
    comm = TorchComm(dist, eng)
    res = {}
    if mode == "p2p":
        run_p2p(rank, world, comm, eng, res)
        np.savez(os.path.join(out_dir, "rank%d.npz" % rank), **res)
        return
    sysm = mac_stokes(dim, n, 0.01)
    f, g = sysm.rhs(0)
    blocks = sysm.facet_blocks() if pre in ("bjac", "bgs", "mypre_a") else None
    ops = DistributedStokes(sysm, blocks, comm, eng, pre=pre if pre in ("bgs", "mypre_a") else None, condense=True,
                            aux_options=AUX if pre == "mypre_a" else None)
    us, ps = ops.local_slices()
    res["slices"] = np.array([us.start, us.stop, ps.start, ps.stop])
    res["n_uncovered"] = ops.n_uncovered
    res["n_interior"] = int(ops.form.interior[us].sum())
    if mode == "cpu":
        # one apply of the partitioned condensed preconditioner step, t1 = (I + E) preA (I + E^T) t0 + A_ii^-1 (I + E^T) t0
        x = np.random.default_rng(11).standard_normal(sysm.n_u)
        y = hipla.Vector(ops.n_u)
        harmonic_extension(hipla.Vector.from_numpy(x[us]), ops.form, 1.7 * ops.preA, result=y)
        res["step"] = y.numpy()
        out = protocol_solve(ops, f, g, tol, maxsteps)
        res.update(out)
    else:                                   # "mailbox": native condensed loop vs the protocol solve of this partition
        ref = protocol_solve(ops, f, g, tol, maxsteps)
        run_ = DistributedBpcg2(sysm, f, g, blocks, dist, eng, comm=comm, pre=pre if pre != "jacobi" else None,
                                transport="mailbox", condense=True, k=ref["k"])
        assert run_.mailbox is not None and run_.native is not None and run_.declined is None
        it, _ = run_.solve(tol=tol, maxsteps=maxsteps, poll_every=16)
        res["hist"], res["it"] = run_.history(it), it
        res["u"], res["p"] = run_.sol[0].numpy(), run_.sol[1].numpy()
        res["timeout"] = int(run_.mailbox.timed_out())
        res["ref_hist"], res["ref_it"], res["k"] = ref["hist"], ref["it"], ref["k"]
        run_.release()
    np.savez(os.path.join(out_dir, "rank%d.npz" % rank), **res)


if __name__ == "__main__":
    a = sys.argv[1:]
    run(int(a[0]), int(a[1]), a[2], a[3], a[4], int(a[5]), int(a[6]), a[7], float(a[8]), int(a[9]))
