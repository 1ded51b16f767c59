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
    """`DistributedStokes(pre="mypre_a")` of every rank of a `world`-way partition."""
    return _simulated_ranks(s, world, engine, pre="mypre_a", aux_options=dict(coarse_size=40))


def _simulated_ranks(s, world, engine, **options):
    """`DistributedStokes(**options)` of every rank of a `world`-way partition, built in this process (the set-up
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
        return DistributedStokes(s, s.line_blocks(3), FakeComm(), engine, **options)

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
        channels, channel = mailbox_channels(layouts)
        assert len(channels) <= P2P_MAX_CHANNELS
        assert list(channel) == ["t1", "aux_x", "aux_e", "aux_y", "vcycle"]
        assert channel["t1"] == 0 and channel["aux_y"] == 0          # t1 and the residual's halo share A's layout: channel 0
        index = list(channel.values())
        numbering.append(index)
        recv = [_recv_layout(h, n) for _, _, h, n in layouts]
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
        mailbox_channels([("n%d" % i, k, None, 1) for i, k in enumerate(keys)])
    chans, channel = mailbox_channels([("t", keys[0], "a", 1), ("u", keys[1], "b", 2), ("v", keys[0], "c", 1)])
    assert chans == [("a", 1), ("b", 2)] and channel == {"t": 0, "u": 1, "v": 0} and list(channel.values()) == [0, 1, 0]
    with pytest.raises(ValueError, match="named"):
        mailbox_channels([("t", keys[0], "a", 1), ("t", keys[1], "b", 2)])


# name -> channel of every configuration the mailbox transport serves, as the positional numbering gave them before the
# entries had names (its `mailbox_layouts` / `mailbox_channels` run on these inputs: the same on every rank of 2 and 3)
CHANNELS_BY_NAME = {
    "plain": {"t1": 0},
    "condensed": {"t1": 0, "cond_lift": 1, "cond_ext": 2},
    "amg": {"t1": 0, "vcycle": 0},
    "amg+bjac": {"t1": 0, "vcycle": 0},
    "mypre_a": {"t1": 0, "aux_x": 1, "aux_e": 2, "aux_y": 0, "vcycle": 3},
}


@pytest.mark.parametrize("world", [2, 3])
@pytest.mark.parametrize("config", sorted(CHANNELS_BY_NAME))
def test_channel_of_every_name_is_the_recorded_number(numpy_engine, world, config):
    from distributed import DistributedAMG, mailbox_channels, mailbox_layouts
    s = mac_stokes(3, 9, 0.01)
    options = {"condensed": dict(condense=True), "mypre_a": dict(pre="mypre_a", aux_options=dict(coarse_size=40))}
    for ops in _simulated_ranks(s, world, numpy_engine, **options.get(config, {})):
        t1, aux = ops.A.operand(), ops.aux
        halo = lambda mat, hv=None: mat.native_halo(hv if hv is not None else mat.operand(), (0, 0))
        condensed = (halo(ops.A), halo(ops.A, t1)) if config == "condensed" else ()
        aux_halos = (halo(aux.transform_t), halo(aux.transform), halo(ops.A, t1)) if aux is not None else None
        V = aux.V if aux is not None else DistributedAMG(s.A, ops.A, coarse_size=40) if config.startswith("amg") else None
        layouts = mailbox_layouts(ops, halo(ops.A, t1), condensed, aux, aux_halos, V, halo(V.A) if V is not None else None)
        channel = mailbox_channels(layouts)[1]
        assert channel == CHANNELS_BY_NAME[config] and list(channel) == list(CHANNELS_BY_NAME[config])


class _Buffer(np.ndarray):
    def data_ptr(self):
        return self.ctypes.data


def _stub_engine(log):
    """The numpy checker engine with what the native set-up asks of the HIP engine: buffers and handles that give a
    pointer, and an ``engine.lib`` that hands out numbered handles and records every destroy call in `log`."""
    import ctypes as C
    import types
    from oracle.numpy_engine import NumpyEngine

    class Lib:
        made = 0

        def __getattr__(self, name):
            def call(*args):
                if name.endswith("_destroy"):
                    log.append((name, args[0].value))
                elif name == "nss_p2p_blob_bytes":
                    args[-1]._obj.value = 16
                elif name in ("nss_dist_create", "nss_dist_amg_create", "nss_dist_aux_create"):
                    Lib.made += 1
                    args[-1]._obj.value = Lib.made
                    log.append((name, Lib.made))
                elif name in ("nss_p2p_create", "nss_p2p_create_vec"):
                    Lib.made += 1
                    args[-2]._obj.value = Lib.made
                    log.append((name, Lib.made))
                return 0
            return call

    class Engine(NumpyEngine):
        stream = None
        lib = Lib()

        def _check(self, status):
            assert status == 0

        def zeros(self, n):
            return super().zeros(n).view(_Buffer)

        def from_host(self, arr):
            return super().from_host(arr).view(_Buffer)

        def csr_create(self, *args, **kw):
            handle = super().csr_create(*args, **kw)
            handle.ptr = None
            return handle

        def amg_create(self, levels, omega):
            return types.SimpleNamespace(ptr=None)

    return Engine()


def test_release_destroys_every_native_handle_once_in_dependency_order():
    """The native handles of a pre="mypre_a" run over the mailbox transport -- made by the run's own set-up steps on a
    stub ``engine.lib`` -- are destroyed exactly once each, in the order mailbox, the loop's dist handle, the
    auxiliary-space term, the V-cycle, the dist handle made for those two: by `release`, and not again by a second
    `release` or by `__del__`."""
    import types
    import hipla
    from distributed import DistributedBpcg2
    log = []
    eng = _stub_engine(log)
    prev = hipla.set_engine(eng)
    try:
        ops = _simulated_mypre_a_ranks(mac_stokes(3, 6, 0.01), 1, eng)[0]
        ops.comm.gather_objects = lambda obj: [obj]
        run = object.__new__(DistributedBpcg2)               # the native set-up steps without the device loop
        run.engine, run.comm, run.ops, run.dist_amg = eng, ops.comm, ops, None
        run.want_transport, run.compact, run.condense = "mailbox", True, False
        run.t1 = ops.A.operand()
        run.loop = types.SimpleNamespace(state=types.SimpleNamespace(p2p=None), keep=[])
        run._native_preconditioner()
        run.enable_mailbox()
        made = dict((name, handle) for name, handle in log)
        assert sorted(made) == ["nss_dist_amg_create", "nss_dist_aux_create", "nss_dist_create", "nss_p2p_create_vec"]
        pre_dist, loop_dist = [handle for name, handle in log if name == "nss_dist_create"]
        assert run.native.handle.value == loop_dist and ops.aux.native.dist.value == pre_dist
        assert run.mailbox_channel_of == [0, 1, 2, 0, 3]
        expected = [("nss_p2p_destroy", made["nss_p2p_create_vec"]), ("nss_dist_destroy", loop_dist),
                    ("nss_dist_aux_destroy", made["nss_dist_aux_create"]),
                    ("nss_dist_amg_destroy", made["nss_dist_amg_create"]), ("nss_dist_destroy", pre_dist)]
        del log[:]
        run.release()
        assert log == expected
        assert run.native is None and run.mailbox is None and run.loop.state.p2p is None
        run.release()
        run.__del__()
        mailbox, aux, V = run.loop.keep[-1], ops.aux, ops.aux.V
        del run, ops
        for obj in (mailbox, aux, V):                        # nor do the objects the handles were made for
            if hasattr(obj, "__del__"):
                obj.__del__()
        assert log == expected
    finally:
        hipla.set_engine(prev)
