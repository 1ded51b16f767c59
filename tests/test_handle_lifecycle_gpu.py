"""Life cycle of the native handles: every device array of a handle is a nss::DeviceBuffer member, so whatever a handle
was walked through -- value codes, row slots, re-plans, the fixed-width copy as an alias or as an own copy, fp32
rounding and narrowing, colourings, condensed operators, the joint AMG cycle -- destroying it gives every allocation
back.  Each case reads nss_device_memory (bytes and number of the library's live device allocations) after
nss_scratch_trim, runs its cycle, destroys the handles, trims, and requires BOTH counts to be back exactly.  Where a step
only changes how a matrix is stored, the product with a fixed random vector keeps its bits.

The storage-form walk goes create -> codes -> slots -> nss_csr_plan_for_pairs -> slots -> ...  On the 512-row
seven-point operator the two row blocks stage far fewer than chunk / 2 columns each, so the matrix is pair-stageable as
uploaded and nss_csr_plan_for_pairs has nothing to re-plan (seen on the device: pair_staged True, generation still 0).
The walk therefore calls nss_csr_plan_for_blocks right behind it, which re-plans for certain: the generation must move,
the slots must go, the codes must stay."""

import ctypes as C
import gc

import numpy as np
import pytest
import scipy.sparse as sp

from staggered_grid import mac_stokes

pytestmark = pytest.mark.gpu


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def round32(m):
    m = sp.csr_matrix(m, copy=True)
    m.data = m.data.astype(np.float32).astype(np.float64)
    return m


def laplace3d(n=8, scale=0.1):
    """seven-point operator on n^3 points: at most 7 entries per row, the values 6 `scale` and -`scale` (not fp32 numbers)"""
    t = sp.diags([-1.0, 2.0, -1.0], [-1, 0, 1], shape=(n, n))
    eye = sp.identity(n)
    L = sp.kron(sp.kron(t, eye), eye) + sp.kron(sp.kron(eye, t), eye) + sp.kron(sp.kron(eye, eye), t)
    L = sp.csr_matrix(scale * L)
    L.sort_indices()
    return L


def two_per_row(rows, seed):
    """row r holds random values in the columns r and r + 1"""
    rng = np.random.default_rng(seed)
    indptr = 2 * np.arange(rows + 1, dtype=np.int32)
    indices = (np.arange(rows)[:, None] + np.array([0, 1])[None, :]).ravel().astype(np.int32)
    return sp.csr_matrix((rng.standard_normal(2 * rows), indices, indptr), shape=(rows, rows + 1))


def tridiagonal(rows):
    return sp.csr_matrix(sp.diags([-1.0, 2.5, -1.0], [-1, 0, 1], shape=(rows, rows)))


def upload(eng, csr, cuts=None):
    csr = sp.csr_matrix(csr)
    csr.sort_indices()
    return eng.csr_create(csr.shape[0], csr.shape[1], csr.indptr, csr.indices, csr.data, cuts=cuts)


def memory(eng):
    """(live bytes, live allocations) of the library with nothing pooled and no forgotten handle of an earlier test"""
    eng.synchronize()
    gc.collect()
    eng.scratch_trim()
    nbytes, count = C.c_int64(-1), C.c_int64(-1)
    eng._check(eng.lib.nss_device_memory(C.byref(nbytes), C.byref(count)))
    return nbytes.value, count.value


def baseline(eng):
    v = eng.zeros(8)
    eng.dot(v, v)                             # (the process-wide reduction scratch is allocated on first use and stays)
    return memory(eng)


def destroy(eng, handle, entry="nss_csr_destroy"):
    """destroy now, and see the return code (the handle's __del__ would swallow it)"""
    ptr, handle.ptr = handle.ptr, None
    assert getattr(eng.lib, entry)(ptr) == 0, eng.lib.nss_last_error()


def spmv(eng, h, x):
    xb, yb = eng.zeros(h.n), eng.zeros(h.m)
    eng.upload(x, xb)
    eng.csr_spmv(h, 1.0, xb, 0.0, yb)
    eng.synchronize()
    return eng.to_host(yb).copy()


def project(eng, h, phi, raw):
    """out = raw - C phi through the fixed-width copy of C (nss_step_project_f64 builds it on first request)"""
    pb, rb, ob = eng.zeros(h.n), eng.zeros(h.m), eng.zeros(h.m)
    eng.upload(phi, pb)
    eng.upload(raw, rb)
    eng._check(eng.lib.nss_step_project_f64(h.ptr, pb.data_ptr(), rb.data_ptr(), ob.data_ptr(), None, 0.0, None, None, 0,
                                            None, eng.stream))
    eng.synchronize()
    return eng.to_host(ob).copy()


def line_jacobi(eng, rows, bs=4):
    """(matrix, block-Jacobi handle over runs of `bs` consecutive dofs that tile the rows): what
    nss_csr_plan_for_blocks plans any matrix with `rows` rows around"""
    assert rows % bs == 0
    D = upload(eng, tridiagonal(rows))
    idx = np.arange(rows, dtype=np.int32).reshape(rows // bs, bs).T
    return D, eng.bjac_create(D, idx)


def test_csr_storage_forms(hip_engine):
    eng = hip_engine
    L = laplace3d()
    assert L.shape == (512, 512) and np.diff(L.indptr).max() == 7 and np.unique(L.data).size == 2
    x = np.random.default_rng(1).standard_normal(L.shape[1])
    start = baseline(eng)
    ends = []
    for _ in range(3):
        with eng.overrides(value_codes=1, fuse_bjac=1):
            a = upload(eng, L)
            y0 = spmv(eng, a, x)
            assert a.code_values() and a.value_bytes() == L.nnz
            assert same_bits(spmv(eng, a, x), y0)
            assert a.plan_row_slots(1)
            assert same_bits(spmv(eng, a, x), y0)
            # re-plans: the slots (positions of the plan that goes) go, the codes (per entry in CSR order) stay
            gen = a.plan_generation()
            a.plan_for_pairs()
            D, J = line_jacobi(eng, a.m)
            assert a.plan_for_blocks(J)
            assert a.plan_generation() > gen
            assert not a.plan_row_slots(None) and a.value_bytes() == L.nnz
            assert same_bits(spmv(eng, a, x), y0)
            assert a.plan_row_slots(1)                               # the slots again, for the new plan
            assert same_bits(spmv(eng, a, x), y0)
            a.drop_value_codes()
            assert a.value_bytes() == 8 * L.nnz and not a.plan_row_slots(None)
            assert same_bits(spmv(eng, a, x), y0)
            eng.csr_round_f32(a)
            twin = upload(eng, round32(L))
            assert same_bits(spmv(eng, a, x), spmv(eng, twin, x))    # (the rounded values, 8 bytes wide)
            eng.csr_narrow_f32(a)
            assert a.value_bytes() == 4 * L.nnz
            ref = round32(L) @ x                                     # (the rule of test_fp32_storage_gpu.py)
            assert np.linalg.norm(spmv(eng, a, x) - ref) <= 1e-14 * np.linalg.norm(ref)
            destroy(eng, J, "nss_bjac_destroy")
            for h in (a, twin, D):
                destroy(eng, h)
        ends.append(memory(eng))
    assert ends == [start] * 3, (start, ends)


@pytest.mark.parametrize("aliases", [True, False], ids=["alias_of_ell", "own_copy"])
def test_fixed_width_copy(hip_engine, aliases):
    """The copy the epilogues read is a view: of ell_col / ell_val where the matrix holds them (the direct-rows threshold
    lowered to its size), of the handle's own copy otherwise.  Rounded once, rebuilt after a re-plan, freed once."""
    eng = hip_engine
    rows = 600
    Cm = two_per_row(rows, 3)
    rng = np.random.default_rng(4)
    phi, raw = rng.standard_normal(rows + 1), rng.standard_normal(rows)
    start = baseline(eng)
    with eng.overrides(direct_rows=1 if aliases else -1, fuse_bjac=1):
        c = upload(eng, Cm)
        assert (c.info()["operand_form"] == "rows") == aliases
        out0, y0 = project(eng, c, phi, raw), spmv(eng, c, phi)
        eng.csr_round_f32(c)
        twin = upload(eng, round32(Cm))
        out32, y32 = project(eng, twin, phi, raw), spmv(eng, twin, phi)
        assert not same_bits(out32, out0)
        assert same_bits(project(eng, c, phi, raw), out32) and same_bits(spmv(eng, c, phi), y32)
        assert not same_bits(y32, y0)
        gen = c.plan_generation()
        D, J = line_jacobi(eng, rows)
        assert c.plan_for_blocks(J) and c.plan_generation() > gen     # one re-plan: every plan form is rebuilt
        assert (c.info()["operand_form"] == "rows") == aliases
        assert same_bits(project(eng, c, phi, raw), out32) and same_bits(spmv(eng, c, phi), y32)
        destroy(eng, J, "nss_bjac_destroy")
        for h in (c, twin, D):
            destroy(eng, h)
    assert memory(eng) == start


def test_block_jacobi_handle(hip_engine):
    """Codes, two colourings in the row-permuted layout, one in the colour-major layout, the condensed operators
    attached, detached and attached again -- all on ONE handle -- then destroy."""
    import hipla
    from hipla import coloring
    eng = hip_engine
    s = mac_stokes(2, 6)
    A = sp.csr_matrix(s.A)
    A.sort_indices()
    n = A.shape[0]
    base = hipla.BlockJacobi._as_table(s.line_blocks(3))[:, :-1]     # (the dofs of the last block stay outside)
    colors = coloring.color_blocks_greedy(coloring.block_graph(A, base))
    order, ptr = coloring.colour_major_order(colors)
    idx = np.ascontiguousarray(base[:, order])
    live = idx.T >= 0
    rowdof = idx.T[live].astype(np.int64)
    ridx = -np.ones(idx.T.shape, dtype=np.int32)
    ridx[live] = np.arange(rowdof.size, dtype=np.int32)
    rows_per_block = live.sum(axis=1)
    block_row0 = np.concatenate([[0], np.cumsum(rows_per_block)])
    color_rowptr = block_row0[ptr]
    n_perm = int(rowdof.size)
    outside = np.setdiff1d(np.arange(n, dtype=np.int64), rowdof)
    assert outside.size > 0
    colmap = np.empty(n, dtype=np.int32)
    colmap[rowdof] = np.arange(n_perm, dtype=np.int32)
    colmap[outside] = n_perm + np.arange(outside.size, dtype=np.int32)
    pos = (np.arange(n_perm, dtype=np.int64) - np.repeat(block_row0[:-1], rows_per_block)).astype(np.uint8)
    rng = np.random.default_rng(7)
    x = rng.standard_normal(n)

    def smooth(j):
        xb, yb = eng.zeros(n), eng.zeros(n)
        eng.upload(x, xb)
        eng.bjac_smooth(j, 1.0, xb, yb, False)
        eng.synchronize()
        return eng.to_host(yb).copy()

    start = baseline(eng)
    with eng.overrides(block_codes=1):
        a = upload(eng, A)
        j = eng.bjac_create(a, idx)
        xb, yb = eng.zeros(n), eng.zeros(n)
        eng.upload(x, xb)
        eng.bjac_apply(j, 1.0, xb, 0.0, yb)
        eng.synchronize()
        y0 = eng.to_host(yb).copy()
        assert j.code_blocks()
        eng.bjac_apply(j, 1.0, xb, 0.0, yb)
        eng.synchronize()
        assert same_bits(eng.to_host(yb), y0)                        # (the coded apply: same doubles, same products)
        rows_perm = eng.csr_select_rows(a, rowdof, cuts=color_rowptr)
        eng.bjac_set_colors(j, rows_perm, ptr, color_rowptr, rowdof, np.ascontiguousarray(ridx.T))
        swept = smooth(j)
        eng.bjac_set_colors(j, rows_perm, ptr, color_rowptr, rowdof, np.ascontiguousarray(ridx.T))
        assert same_bits(smooth(j), swept)
        full_perm = eng.csr_permute(a, rowdof, colmap, n_perm + max(1, outside.size), cuts=color_rowptr, max_rows=256,
                                    row_pos=pos)
        eng.bjac_set_colors_permuted(j, full_perm, ptr, color_rowptr, rowdof, np.ascontiguousarray(ridx.T))
        assert same_bits(smooth(j), swept)                           # (same colours: both layouts give the same bits)
        # the condensed operators: only their shapes are checked at attach, and nothing here launches with them
        square = upload(eng, sp.identity(n, format="csr"))
        htp = upload(eng, sp.eye(n_perm, n, format="csr"))
        hp = upload(eng, sp.eye(outside.size, n_perm + outside.size, format="csr"))
        dinner = np.ones(outside.size)
        attach = lambda: eng.lib.nss_bjac_set_condensed(j.ptr, square.ptr, square.ptr, square.ptr, square.ptr, htp.ptr,
                                                        hp.ptr, dinner.ctypes.data)
        detach = lambda: eng.lib.nss_bjac_set_condensed(j.ptr, None, None, None, None, None, None, None)
        held = memory(eng)
        assert attach() == 0, eng.lib.nss_last_error()
        attached = memory(eng)
        assert attached == (held[0] + 8 * outside.size, held[1] + 1)
        assert detach() == 0 and memory(eng) == held
        assert attach() == 0 and memory(eng) == attached
        assert same_bits(smooth(j), swept)
        destroy(eng, j, "nss_bjac_destroy")
        for h in (a, rows_perm, full_perm, square, htp, hp):
            destroy(eng, h)
    assert memory(eng) == start


def test_amg_auxiliary_and_fdm_handles(hip_engine):
    """A hierarchy on the 8 x 8 x 8 operator, the auxiliary-space term over two components that share it (the joint
    cycle: the hierarchy is re-planned in place, descriptors and interleaved work vectors are added), an FDM handle."""
    import hipla
    from hipla import amg, fdm
    eng = hip_engine
    L = laplace3d()
    n = L.shape[0]
    start = baseline(eng)
    V = amg.SmoothedAggregationAMG(hipla.SparseMatrix.from_scipy(L), coarse_size=40)
    assert len(V.levels) >= 2
    hierarchy = memory(eng)
    assert hierarchy[0] > start[0] and hierarchy[1] > start[1]
    T = hipla.SparseMatrix.from_scipy(sp.identity(2 * n, format="csr"))
    aux = amg.AuxiliarySpaceAMG(T, [V, V])
    b, y = eng.zeros(2 * n), eng.zeros(2 * n)
    eng.upload(np.random.default_rng(9).standard_normal(2 * n), b)
    eng.amg_apply(aux.handle, 1.0, b, y)
    eng.synchronize()
    assert np.isfinite(eng.to_host(y)).all()
    destroy(eng, aux.handle, "nss_amg_destroy")
    del aux, T
    # (what the joint cycle's re-plan left in the shared hierarchy is the hierarchy's: it goes with it)
    destroy(eng, V.handle, "nss_amg_destroy")
    del V
    assert memory(eng) == start

    factors, why = fdm.fdm_factors(L, (8, 8, 8))
    assert factors is not None, why
    h = fdm.create_handle(eng, factors)
    cells = 8 * 8 * 8
    assert memory(eng) == (start[0] + 8 * (3 * 8 * 8 + 3 * 8 + 2 * cells), start[1] + 6)
    destroy(eng, h, "nss_fdm_destroy")
    assert memory(eng) == start


def test_replan_through_a_shared_handle(hip_engine):
    """nss_csr_plan_for_blocks re-plans a matrix somebody else holds too, leaves the arrays of the Jacobi-block plan set,
    and a second call finds them: nothing is allocated, the plan stays."""
    eng = hip_engine
    rows = 600
    Cm = two_per_row(rows, 11)
    x = np.random.default_rng(12).standard_normal(rows + 1)
    start = baseline(eng)
    with eng.overrides(fuse_bjac=1):
        c = upload(eng, Cm)
        other = c                                                    # (the second holder: the same native handle)
        y0 = spmv(eng, c, x)
        gen = c.plan_generation()
        D, J = line_jacobi(eng, rows)
        assert c.plan_for_blocks(J)
        planned, gen1 = memory(eng), other.plan_generation()
        assert gen1 > gen
        assert other.plan_for_blocks(J)                              # already planned around this handle: a no-op
        assert memory(eng) == planned and other.plan_generation() == gen1
        assert same_bits(spmv(eng, other, x), y0)
        destroy(eng, J, "nss_bjac_destroy")
        for h in (c, D):
            destroy(eng, h)
    assert memory(eng) == start
