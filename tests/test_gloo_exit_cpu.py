"""Ranks of a gloo process group that end without `destroy_process_group()` (tests/condensed_dist_worker.py does): the
group is then torn down during interpreter shutdown, where a rank that had finished its work can end in std::terminate
("terminate called without an active exception", exit status -6) -- intermittently, more often the busier the host.
`distributed.TorchComm` destroys a gloo group in an exit handler instead.  Checked here: ranks that leave the group alone
exit with status 0, a rank whose peer is already gone does not block in the handler, and a caller that destroyed the
group itself is not disturbed."""

import os
import subprocess
import sys
import tempfile

import pytest

from conftest import PKG, ROOT

WORKER = r"""
import os, sys, time
sys.path[:0] = [%r, %r]
rank, world, init_file, ending = int(sys.argv[1]), int(sys.argv[2]), sys.argv[3], sys.argv[4]
import numpy as np
import torch.distributed as dist
dist.init_process_group("gloo", init_method="file://" + init_file, rank=rank, world_size=world)
from oracle.numpy_engine import NumpyEngine
import distributed
comm = distributed.TorchComm(dist, NumpyEngine())
buf = np.full(4, rank + 1.0)
comm.allreduce_sum(buf)
assert buf[0] == world * (world + 1) / 2
assert distributed._exit_hooked
if ending == "peer-dies" and rank == 1:
    os._exit(0)                      # gone without any teardown
if ending == "peer-dies":
    time.sleep(1.0)                  # the peer is gone by the time this rank's exit handler runs
if ending == "destroyed":
    dist.destroy_process_group()
print("finished", rank)
""" % (ROOT, PKG)


@pytest.mark.parametrize("ending", ["left-alone", "peer-dies", "destroyed"])
def test_gloo_ranks_exit_cleanly(ending):
    tmp = tempfile.mkdtemp(prefix="nssexit_")
    env = dict(os.environ, OMP_NUM_THREADS="1")
    procs = [subprocess.Popen([sys.executable, "-c", WORKER, str(r), "2", os.path.join(tmp, "rendezvous"), ending], env=env,
                              stdout=subprocess.PIPE, stderr=subprocess.STDOUT) for r in range(2)]
    try:
        for r, p in enumerate(procs):
            out, _ = p.communicate(timeout=120)          # (a handler that blocked would end here)
            text = out.decode(errors="replace")
            assert p.returncode == 0, text[-2000:]
            assert "terminate called" not in text
            if not (ending == "peer-dies" and r == 1):
                assert "finished %d" % r in text
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
