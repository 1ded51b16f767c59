"""Worker of test_mailbox_precond_gpu.py: one rank of `world` processes, all on the one visible GPU, gloo set-up
communicator, the native partitioned loops over the mailbox transport (csrc/p2p.h).

mode "vec":   the transport's vector all-reduce on several contribution-range layouts, three calls each.
mode "solve": DistributedBpcg2(pre=..., transport="mailbox") -- the V-cycle / auxiliary-space term natively inside
              the loop -- plus, for "mypre_a", the native auxiliary apply of a fixed vector."""

import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "navier-stokes-solver_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

VEC_N = 1000


def vec_cases(world):
    """(name, lo[], hi[]) per case: overlapping ranges, one rank with an empty range, every rank the full range."""
    step = VEC_N // (world + 1)
    overlap = ([q * step for q in range(world)], [min(VEC_N, (q + 2) * step + 7) for q in range(world)])
    empty = ([q * step for q in range(world)], [min(VEC_N, (q + 2) * step) for q in range(world)])
    empty[1][world // 2] = empty[0][world // 2]
    full = ([0] * world, [VEC_N] * world)
    return [("overlap",) + overlap, ("empty",) + empty, ("full",) + full]


def contribution(rank, call, lo, hi):
    """What rank `rank` contributes in call `call`: zero outside its range (the transport reads the range only)."""
    v = np.zeros(VEC_N)
    x = np.random.default_rng(1000 * rank + call).standard_normal(VEC_N) * 10.0 ** (rank % 3)
    v[lo:hi] = x[lo:hi]
    return v, x


def run_vec(rank, world, eng, comm, res):
    import torch
    from distributed import DistributedStokes, MailboxTransport
    from staggered_grid import mac_stokes
    ops = DistributedStokes(mac_stokes(2, 12, 0.01), None, comm, eng)
    probe = ops.A.operand()
    for name, lo, hi in vec_cases(world):
        mb = MailboxTransport(comm, eng, [(ops.A.native_halo(probe, (0, 0)), ops.n_u)], vector=(VEC_N, lo, hi))
        for call in range(3):                       # both zone copies, and the first one again
            _, x = contribution(rank, call, lo[rank], hi[rank])
            src = torch.tensor(x, dtype=torch.float64, device=eng.device)   # garbage outside the range: not read
            dst = torch.full((VEC_N,), np.nan, dtype=torch.float64, device=eng.device)
            mb.allreduce_vec(src, dst)
            res["%s_%d" % (name, call)] = dst.cpu().numpy()
        res["%s_seq" % name] = mb.counters()[0]
        res["%s_timeout" % name] = int(mb.timed_out())
        mb.close()


def run_solve(rank, world, eng, comm, dist, res, dim, n, pre, tol, maxsteps):
    import hipla
    from distributed import DistributedBpcg2
    from staggered_grid import mac_stokes
    sysm = mac_stokes(dim, n, 0.01)
    f, g = sysm.rhs(0)
    aux_options = dict(coarse_size=40) if pre == "mypre_a" else None
    run = DistributedBpcg2(sysm, f, g, sysm.line_blocks(3), dist, eng, comm=comm, pre=pre, transport="mailbox",
                           aux_options=aux_options)
    res["native"] = int(run.native is not None)
    res["mailbox"] = int(run.mailbox is not None)
    res["declined"] = str(run.declined)
    res["channels"] = np.array(run.mailbox_channel_of)
    us, _ = run.ops.local_slices()
    if pre == "mypre_a":
        aux = run.ops.aux
        res["aux_levels"] = np.array(aux.level_sizes)
        x = np.random.default_rng(9).standard_normal(sysm.n_u)
        y = hipla.Vector(run.ops.n_u)
        aux.native_apply(1.0, hipla.Vector.from_numpy(x[us]), y)     # over the transport: every rank calls it
        res["aux_apply"] = y.numpy()
    it, conv = run.solve(tol=tol, maxsteps=maxsteps, poll_every=16)
    res["it"], res["conv"] = it, int(conv)
    res["hist"] = run.history(it)
    res["u"] = run.sol[0].numpy()
    res["timeout"] = int(run.mailbox.timed_out())
    run.release()
    # per-phase device times of the first iterations of a fresh run (profiles/mailbox_precond.md)
    run = DistributedBpcg2(sysm, f, g, sysm.line_blocks(3), dist, eng, comm=comm, pre=pre, transport="mailbox",
                           aux_options=aux_options)
    run.start(tol, maxsteps)
    prof, nprof = run.profile(0, 12)
    res["profile_names"] = np.array(list(prof))
    res["profile_ms"] = np.array([prof[k] for k in prof])
    res["profile_n"] = nprof
    res["timeout_after_profile"] = int(run.mailbox.timed_out())
    run.release()


def main(rank, world, init_file, out_dir, mode, dim, n, pre, tol, maxsteps):
    import torch
    import torch.distributed as dist
    dist.init_process_group("gloo", init_method="file://" + init_file, rank=rank, world_size=world)
    import hipla
    torch.cuda.set_device(0)
    hipla.set_engine(None)
    eng = hipla.get_engine()
    from distributed import TorchComm
    comm = TorchComm(dist, eng)
    res = {}
    if mode == "vec":
        run_vec(rank, world, eng, comm, res)
    else:
        run_solve(rank, world, eng, comm, dist, res, dim, n, pre, tol, maxsteps)
    np.savez(os.path.join(out_dir, "rank%d.npz" % rank), **res)
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    a = sys.argv[1:]
    main(int(a[0]), int(a[1]), a[2], a[3], a[4], int(a[5]), int(a[6]), a[7], float(a[8]), int(a[9]))
