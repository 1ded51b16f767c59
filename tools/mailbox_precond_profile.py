"""Per-rank device time per iteration of BPCG v2 with pre="mypre_a" over the mailbox transport (2 processes on ONE
GPU, tests/mailbox_precond_worker.py) next to the 1-rank RCCL run of the same system (the native loop's per-phase
profile, nss_dist_profile_*), and the traffic of the coarse vector all-reduce: sum_q (hi_q - lo_q) / nc of the
V-cycles' contribution ranges with `slabs` simulated slabs (CPU only).  Neither is cross-GPU evidence: processes
sharing one GPU see no xGMI link.

    python tools/mailbox_precond_profile.py profile [dim n]      (GPU)
    python tools/mailbox_precond_profile.py ranges [dim n slabs]  (CPU)"""
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "navier-stokes-solver_amd"))


def ranges(dim, n, slabs):
    import scipy.sparse as sp
    import hipla
    from oracle.numpy_engine import NumpyEngine
    from distributed import coarse_contribution_ranges
    from hipla.amg import build_hierarchy
    from staggered_grid import mac_stokes
    hipla.set_engine(NumpyEngine())
    s = mac_stokes(dim, n, 0.01)
    vel, _ = s.partition(slabs)
    st = s.auxiliary_space_stacked()
    node = np.asarray(st["node_slab_offsets"], dtype=np.int64)[np.searchsorted(s.velocity_slab_offsets, vel)]
    out = {}
    for name, mat, offs in (("amg (A)", s.A, vel), ("mypre_a (nodal Laplacian)", st["laplacian"], node)):
        R = build_hierarchy(hipla.SparseMatrix.from_scipy(sp.csr_matrix(mat)))[0]["R"].to_scipy()
        lo, hi = coarse_contribution_ranges(R, offs)
        out[name] = dict(nc=int(R.shape[0]), fraction=float(np.sum(hi - lo)) / R.shape[0],
                         per_rank=[int(h - l) for l, h in zip(lo, hi)])
    return dict(dim=dim, n=n, slabs=slabs, ranges=out)


def profile(dim, n):
    import torch.distributed as dist
    from distributed import DistributedBpcg2
    from rccl_comm import RcclComm
    from staggered_grid import mac_stokes
    tmp = tempfile.mkdtemp(prefix="nssmbxprof_")
    worker = os.path.join(ROOT, "tests", "mailbox_precond_worker.py")
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", OMP_NUM_THREADS="1", HSA_ENABLE_IPC_MODE_LEGACY="0")
    procs = [subprocess.Popen([sys.executable, worker, str(r), "2", os.path.join(tmp, "rdv"), tmp, "solve", str(dim),
                               str(n), "mypre_a", "1e-8", "3000"], env=env) for r in range(2)]
    for p in procs:
        if p.wait(timeout=600) != 0:
            raise SystemExit("worker failed")
    out = {}
    for r in range(2):
        d = np.load(os.path.join(tmp, "rank%d.npz" % r))
        out["mailbox_2ranks_rank%d" % r] = dict(zip([str(k) for k in d["profile_names"]], map(float, d["profile_ms"])))
    import hipla
    hipla.set_engine(None)
    eng = hipla.get_engine()
    s = mac_stokes(dim, n, 0.01)
    f, g = s.rhs(0)
    dist.init_process_group("gloo", init_method="file://" + os.path.join(tmp, "rdv1"), rank=0, world_size=1)
    comm = RcclComm(dist, eng)
    run = DistributedBpcg2(s, f, g, s.line_blocks(3), dist, eng, comm=comm, pre="mypre_a", aux_options=dict(coarse_size=40))
    run.start(1e-8, 3000)
    prof, _ = run.profile(0, 12)
    out["rccl_1rank"] = prof
    run.release()
    comm.close()
    dist.destroy_process_group()
    for k, v in out.items():
        v["total"] = sum(v.values())
    return dict(dim=dim, n=n, iterations=12, ms_per_iteration=out)


if __name__ == "__main__":
    a = sys.argv[1:]
    if a and a[0] == "ranges":
        dim, n, slabs = (int(v) for v in (a[1:4] if len(a) > 3 else (3, 136, 8)))
        print(json.dumps(ranges(dim, n, slabs)))
    else:
        dim, n = (int(v) for v in (a[1:3] if len(a) > 2 else (3, 10)))
        print(json.dumps(profile(dim, n)))
