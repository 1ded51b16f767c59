"""Host-side bookkeeping of the V-cycle and the auxiliary-space term over the mailbox transport: the contribution
ranges of the coarse all-reduce and the channel assignment of the halos, for every rank of simulated partitions."""

import numpy as np
import pytest
import scipy.sparse as sp

from staggered_grid import mac_stokes


@pytest.mark.parametrize("world", [2, 3, 5, 8])
def test_contribution_ranges_cover_every_nonempty_row(numpy_engine, world):
    """[lo_q, hi_q) of rank q holds every non-empty row of its share R[:, slab q] of the restriction, and is tight."""
    from distributed import coarse_contribution_ranges
    from hipla import SparseMatrix
    from hipla.amg import build_hierarchy
    s = mac_stokes(3, 10, 0.01)
    vel, _ = s.partition(world)
    st = s.auxiliary_space_stacked()
    slab = np.searchsorted(s.velocity_slab_offsets, vel)
    node = np.asarray(st["node_slab_offsets"], dtype=np.int64)[slab]
    for mat, offs in ((s.A, vel), (st["laplacian"], node)):
        R = build_hierarchy(SparseMatrix.from_scipy(sp.csr_matrix(mat), engine=numpy_engine), coarse_size=40)[0]["R"].to_scipy()
        lo, hi = coarse_contribution_ranges(R, offs)
        assert lo.shape == hi.shape == (world,)
        for q in range(world):
            share = sp.csr_matrix(R[:, offs[q]:offs[q + 1]])
            rows = np.flatnonzero(np.diff(share.indptr))
            if rows.size == 0:
                assert lo[q] == hi[q]
                continue
            assert lo[q] == rows[0] and hi[q] == rows[-1] + 1
            assert 0 <= lo[q] < hi[q] <= R.shape[0]
        total = int(np.sum(hi - lo))
        assert total <= world * R.shape[0]


def _simulated_mypre_a_ranks(s, world, engine):
    """`DistributedStokes(pre="mypre_a")` of every rank of a `world`-way partition, built in this process (the set-up
    all-gathers of halo requests recorded in a first pass and replayed in a second)."""
    from distributed import DistributedStokes
    recorded = [[] for _ in range(world)]

    def build(rank, replay):
        class FakeComm:
            size = world

            def __init__(self):
                self.calls = 0

            def gather_requests(self, mine, compute):
                k, self.calls = self.calls, self.calls + 1
                if not replay:
                    recorded[rank].append(mine)
                    return [compute(q) for q in range(world)]
                return [recorded[q][k] for q in range(world)]

        FakeComm.rank = rank
        return DistributedStokes(s, s.line_blocks(3), FakeComm(), engine, pre="mypre_a", aux_options=dict(coarse_size=40))

    for rank in range(world):
        build(rank, False)
    return [build(rank, True) for rank in range(world)]


def _recv_layout(halo, n_owned):
    keep = halo._keep[0]
    return (int(n_owned), tuple(keep["h_recv_peer"]), tuple(keep["h_recv_off"]), tuple(keep["h_recv_cnt"]))


@pytest.mark.parametrize("world", [2, 3])
def test_mypre_a_channels_separate_distinct_layouts(numpy_engine, world):
    """The halos of a pre="mypre_a" run over the mailbox transport -- t1, transform.T's operand, transform's operand,
    t1 for the residual, the nodal Laplacian's operand -- get one channel per operand layout: halos on one channel have
    the same receive layout on every rank, distinct layouts get distinct channels, every rank numbers them alike, and
    they fit the transport's channel count."""
    from distributed import P2P_MAX_CHANNELS, mailbox_channels, mailbox_layouts
    s = mac_stokes(3, 9, 0.01)
    numbering = []
    for ops in _simulated_mypre_a_ranks(s, world, numpy_engine):
        aux = ops.aux
        t1 = ops.A.operand()
        halo_t1 = ops.A.native_halo(t1, (0, 0))
        hx = aux.transform_t.native_halo(aux.transform_t.operand(), (0, 0))
        he = aux.transform.native_halo(aux.transform.operand(), (0, 0))
        hy = ops.A.native_halo(t1, (0, 0))
        hv = aux.L.native_halo(aux.L.operand(), (0, 0))
        layouts = mailbox_layouts(ops, halo_t1, (), aux, (hx, he, hy), aux.V, hv)
        channels, index = mailbox_channels(layouts)
        assert len(channels) <= P2P_MAX_CHANNELS
        assert index[0] == 0 and index[3] == 0          # t1 and the residual's halo share A's layout: channel 0
        numbering.append(index)
        recv = [_recv_layout(h, n) for _, h, n in layouts]
        for i in range(len(layouts)):
            for j in range(len(layouts)):
                if index[i] == index[j]:
                    assert recv[i] == recv[j]
                elif recv[i] != recv[j]:
                    assert index[i] != index[j]
        for c, (h, n) in enumerate(channels):           # the transport is created with the first halo of each channel
            assert _recv_layout(h, n) == recv[index.index(c)]
    assert all(ix == numbering[0] for ix in numbering)
    assert numbering[0] == [0, 1, 2, 0, 3]


def test_channel_count_is_bounded():
    from distributed import P2P_MAX_CHANNELS, mailbox_channels
    keys = [object() for _ in range(P2P_MAX_CHANNELS + 1)]
    with pytest.raises(ValueError, match="at most"):
        mailbox_channels([(k, None, 1) for k in keys])
    chans, index = mailbox_channels([(keys[0], "a", 1), (keys[1], "b", 2), (keys[0], "c", 1)])
    assert chans == [("a", 1), ("b", 2)] and index == [0, 1, 0]
