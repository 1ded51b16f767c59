"""The device set-up kernels on inputs the grid matrices never produce (setup_cases.py) against references that no engine is
behind (setup_reference.py, oracle/krylov_ref.py::sa_*):

  bjac_setup_kernel / bjac_pack_sym_kernel (csrc/precond.hip)   row swaps, zero diagonals, padding anywhere in the column,
      the 1e-12 symmetry decision from both sides, singular blocks -- J x against the long-double block solve,
      |y_i - y_ld_i| <= GAMMA * 2^-53 * E_i with E = |A_bb^-1| |A_bb| |A_bb^-1| |x_b|;
  nss_csr_spgemm, nss_csr_transpose, nss_amg_aggregate, nss_amg_prolongator, nss_csr_select_rows, nss_csr_permute
      (csrc/amg_setup.hip)   sums that cancel, key widths at powers of two, single-row and empty chunks, threshold ties,
      one-sided strength, 86 Luby rounds, unsorted rows -- bit for bit, in stored order where the operation keeps it.

Every case first asserts the situation it is there for."""

import numpy as np
import pytest
import scipy.sparse as sp

import amg_cycle_reference as cyc
import setup_cases as cases
import setup_reference as sr

pytestmark = pytest.mark.gpu


def _assert_situation(name, situation):
    missing = [what for what, holds in situation.items() if not holds]
    assert not missing, "%s does not contain: %s" % (name, "; ".join(missing))


def _same_arrays(engine, handle, rowptr, col, val, shape, what=""):
    """the handle holds exactly these arrays, in this order"""
    got_rowptr, got_col, got_val = engine.csr_to_host(handle)
    assert (handle.m, handle.n, handle.nnz) == (shape[0], shape[1], len(col)), what
    np.testing.assert_array_equal(got_rowptr, rowptr, err_msg=what)
    np.testing.assert_array_equal(got_col, col, err_msg=what)
    np.testing.assert_array_equal(got_val, val, err_msg=what)                  # bit-identical ...
    np.testing.assert_array_equal(np.signbit(got_val), np.signbit(val), err_msg=what)   # ... signed zeros included


def _same_csr(engine, handle, ref, what=""):
    ref = sp.csr_matrix(ref)
    ref.sort_indices()
    _same_arrays(engine, handle, ref.indptr, ref.indices, ref.data, ref.shape, what)


def _upload(A):
    import hipla
    return hipla.SparseMatrix.from_scipy(sp.csr_matrix(A))


# ---- block Jacobi --------------------------------------------------------------------------------------------------------
def _storage(engine, J):
    """(packed?, run table? or None where the handle does not show it, doubles per dictionary entry or 0) from the bytes one
    apply streams (nss_bjac_block_codes): 8 bytes per stored inverse entry, 4 per index word"""
    bs, nb, n = J.bs, J.nblocks, J.n
    with engine.overrides(block_codes=0):
        per_block, rest = divmod(J.handle.block_codes()[1] - 16 * n, nb)
    assert rest == 0
    full, tri = 8 * bs * bs, 4 * bs * (bs + 1)
    assert per_block in ((full + 4 * bs, tri + 4 * bs, tri + 4) if bs > 1 else (full + 4 * bs,)), per_block
    packed = bs > 1 and per_block != full + 4 * bs
    run = (per_block == tri + 4) if packed else None
    doubles = 0
    if J.block_coded:
        n_codes, dict_ = J.handle.block_codes()[0], J.handle.download_block_codes()[1]
        doubles = dict_.shape[1]
        with engine.overrides(block_codes=1):
            index, rest = divmod(J.handle.block_codes()[1] - 16 * n - 8 * n_codes * doubles - nb, nb)
        assert rest == 0 and index in (4, 4 * bs)
        run = index == 4 if bs > 1 else run
    return packed, run, doubles


@pytest.mark.parametrize("name", list(cases.BJAC_BUILDERS))
def test_block_jacobi_against_the_long_double_solve(hip_engine, name):
    import hipla
    eng = hip_engine
    case = cases.bjac_case(name)
    _assert_situation(name, case.situation)
    J = hipla.BlockJacobi(_upload(case.A), case.idx)
    packed, run, doubles = _storage(eng, J)
    bs = case.idx.shape[0]
    assert packed == case.packed, "storage: %s, the case declares %s" % (("full", "packed")[packed], ("full", "packed")[case.packed])
    assert bool(J.block_coded) == case.coded
    assert run is None or run == case.run
    if J.block_coded:
        assert doubles == (bs * (bs + 1) // 2 if case.packed else bs * bs)
    xs, y0 = cases.bjac_vectors(case)
    free = ~sr.covered(case.idx, case.n)
    worst = 0.0
    for code_mode in (0, 1) if J.block_coded else (0,):
        with eng.overrides(block_codes=code_mode):
            for x in xs:
                want, bound = sr.block_solve_ld(case.A, case.idx, x), sr.block_bound(case.A, case.idx, x)
                xd, yd = hipla.Vector.from_numpy(x), hipla.Vector.from_numpy(np.full(case.n, 7.0))
                J.Mult(xd, yd)
                got = yd.numpy()
                assert np.all(got[free] == 0.0)
                r = sr.ratio(got, want, bound)
                assert r <= sr.GAMMA, "%s Mult (codes %d): |err_i| / (2^-53 E_i) reaches %.3g" % (name, code_mode, r)
                worst = max(worst, r)
                yd = hipla.Vector.from_numpy(y0)
                J.MultAdd(-0.5, xd, yd)
                got = yd.numpy()
                np.testing.assert_array_equal(got[free], y0[free])
                r = sr.ratio(got, y0.astype(sr.LD) - 0.5 * want, np.abs(y0).astype(sr.LD) + 0.5 * bound)
                assert r <= sr.GAMMA, "%s MultAdd (codes %d): ratio %.3g" % (name, code_mode, r)
                worst = max(worst, r)
    print("%s: kernel |err_i| / (2^-53 E_i) <= %.4g (GAMMA %.4g); %s%s" % (
        name, worst, sr.GAMMA, ("full", "packed")[packed], ", coded" if J.block_coded else ""))


@pytest.mark.parametrize("name", list(cases.BJAC_SINGULAR))
def test_singular_blocks_are_counted_and_the_engine_goes_on(hip_engine, name):
    import hipla
    from hipla.hip_engine import NssError
    case = cases.bjac_case(name)
    _assert_situation(name, case.situation)
    with pytest.raises(NssError, match="%d singular" % case.singular):
        hipla.BlockJacobi(_upload(case.A), case.idx)
    good = cases.bjac_case("swap_2x2[1]")
    J = hipla.BlockJacobi(_upload(good.A), good.idx)
    x = cases.bjac_vectors(good)[0][0]
    y = hipla.Vector(good.n)
    J.Mult(hipla.Vector.from_numpy(x), y)
    assert sr.ratio(y.numpy(), sr.block_solve_ld(good.A, good.idx, x), sr.block_bound(good.A, good.idx, x)) <= sr.GAMMA


# ---- sparse products -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(cases.SPGEMM_BUILDERS))
def test_spgemm_edges(hip_engine, name):
    from oracle import krylov_ref as kr
    case = cases.spgemm_case(name)
    _assert_situation(name, case.situation)
    ref = kr.sa_spgemm(case.X, case.Y)
    Xd, Yd = _upload(case.X), _upload(case.Y)
    for cap in cases.CAPS:                                     # one pass / every row its own chunk / a few rows per chunk
        C = hip_engine.csr_spgemm(Xd.handle, Yd.handle, cap)
        _same_csr(hip_engine, C, ref, "%s cap=%d" % (name, cap))
        if case.integer:
            _same_csr(hip_engine, C, sp.csr_matrix(case.X.toarray() @ case.Y.toarray()), "%s cap=%d, dense" % (name, cap))
        assert C.nnz == case.figures["stored"]


# ---- transpose -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m,n", cases.TRANSPOSE_SHAPES)
def test_transpose_edges(hip_engine, m, n):
    M, situation = cases.transpose_case(m, n)
    _assert_situation("transpose %dx%d" % (m, n), situation)
    T = hip_engine.csr_transpose(_upload(M).handle)
    _same_arrays(hip_engine, T, *sr.transpose_stable(M.indptr, M.indices, M.data, M.shape))


def test_transpose_of_unsorted_rows(hip_engine):
    eng = hip_engine
    seen = 0
    for case in cases.all_permute_cases():
        if "wide" not in case.name and "local" not in case.name:
            continue
        rowptr, col, val, shape = sr.permute_rows_cols(case.source, case.rows, case.colmap, case.ncols_out)
        seen += any(np.any(np.diff(col[a:b]) < 0) for a, b in zip(rowptr[:-1], rowptr[1:]))
        P = eng.csr_permute(_upload(case.source).handle, case.rows, case.colmap, case.ncols_out)
        trow, tcol, tval, tshape = sr.transpose_stable(rowptr, col, val, shape)
        _same_arrays(eng, eng.csr_transpose(P), trow, tcol, tval, tshape, case.name)
        assert all(np.all(np.diff(tcol[a:b]) > 0) for a, b in zip(trow[:-1], trow[1:]))      # source rows ascending
    assert seen >= 8


# ---- aggregation and prolongator -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(cases.AGG_BUILDERS))
def test_aggregation_edges(hip_engine, name):
    from oracle import krylov_ref as kr
    case = cases.agg_case(name)
    _assert_situation(name, case.situation)
    Ad = _upload(case.A)
    ref_agg, ref_n = kr.sa_aggregate(case.A, case.theta, case.priority)
    agg, nagg = hip_engine.amg_aggregate(Ad.handle, case.theta, case.priority)
    assert nagg == ref_n == case.figures["aggregates"]
    np.testing.assert_array_equal(hip_engine.index_to_host(agg), ref_agg)
    if case.prolongate:
        for omega in (2.0 / 3.0, 1.0):
            P = hip_engine.amg_prolongator(Ad.handle, agg, nagg, omega)
            _same_csr(hip_engine, P, kr.sa_prolongator(case.A, ref_agg, ref_n, omega), "%s omega=%g" % (name, omega))


@pytest.mark.parametrize("name", list(cases.PRO_BUILDERS))
def test_prolongator_exact_entries(hip_engine, name):
    from oracle import krylov_ref as kr
    case = cases.PRO_BUILDERS[name]()
    _assert_situation(name, case.situation)
    agg = hip_engine.torch.from_numpy(case.agg).to(hip_engine.device)
    P = hip_engine.amg_prolongator(_upload(case.A).handle, agg, case.nagg, case.omega)
    _same_csr(hip_engine, P, kr.sa_prolongator(case.A, case.agg, case.nagg, case.omega), name)


@pytest.mark.parametrize("bad_id", ["nagg", -1])
def test_prolongator_refuses_an_aggregate_id_out_of_range(hip_engine, bad_id):
    from hipla.hip_engine import NssError
    from oracle import krylov_ref as kr
    case = cases.PRO_BUILDERS["isolated_unit_omega"]()
    Ad = _upload(case.A)
    wrong = case.agg.copy()
    wrong[5] = case.nagg if bad_id == "nagg" else -1
    with pytest.raises(NssError, match="aggregate id out of range"):
        hip_engine.amg_prolongator(Ad.handle, hip_engine.torch.from_numpy(wrong).to(hip_engine.device), case.nagg, case.omega)
    agg = hip_engine.torch.from_numpy(case.agg).to(hip_engine.device)
    _same_csr(hip_engine, hip_engine.amg_prolongator(Ad.handle, agg, case.nagg, case.omega),
              kr.sa_prolongator(case.A, case.agg, case.nagg, case.omega))


# ---- select and permute ----------------------------------------------------------------------------------------------------
def _check_spmv(engine, handle, rowptr, col, val, shape, what):
    """one SpMV through the handle's index form against the long-double row sums of the arrays as stored"""
    ref = sr.as_stored(rowptr, col, val, shape)
    x = np.random.default_rng(shape[0] + 3 * shape[1]).standard_normal(shape[1])
    xd, yd = engine.from_host(x), engine.from_host(np.full(shape[0], 7.0))
    engine.csr_spmv(handle, 1.0, xd, 0.0, yd)
    cyc.check(engine.to_host(yd), cyc.spmv_ld(ref, x), cyc.spmv_ld(cyc._abs(ref), np.abs(x)),
              2.0 * cyc.U64 * (cyc.longest_row(ref) + 3), what)


@pytest.mark.parametrize("source", ["ragged", "stokes"])
def test_permute_edges(hip_engine, source):
    eng = hip_engine
    A = cases.permute_sources()[source]
    Ad = _upload(A)
    for case in cases.permute_cases(source, A):
        rowptr, col, val, shape = sr.permute_rows_cols(A, case.rows, case.colmap, case.ncols_out)
        h = eng.csr_permute(Ad.handle, case.rows, case.colmap, case.ncols_out, case.cuts, case.max_rows, case.row_pos)
        _same_arrays(eng, h, rowptr, col, val, shape, case.name)
        broken = sr.plan_respects(h.row_blocks(), case.cuts, case.max_rows, case.row_pos)
        assert broken is None, "%s: %s" % (case.name, broken)
        info = h.info()
        print("%s: %d row blocks, index_bytes %d, %s" % (case.name, info["row_blocks"], info["index_bytes"], info["operand_form"]))
        if case.index_bytes is not None:
            assert info["index_bytes"] == case.index_bytes, case.name
        if case.rows.size:
            _check_spmv(eng, h, rowptr, col, val, shape, case.name)


@pytest.mark.parametrize("source", ["ragged", "stokes"])
def test_select_rows_edges(hip_engine, source):
    eng = hip_engine
    A = cases.permute_sources()[source]
    Ad = _upload(A)
    m = A.shape[0]
    rng = np.random.default_rng(m)
    picks = {"permutation": rng.permutation(m), "subset": rng.permutation(m)[: m // 2], "repeats": rng.integers(0, m, m + 9),
             "none": np.zeros(0, dtype=np.int64)}
    for what, rows in picks.items():
        k = rows.size
        for cuts in (None, [0], [k], [0, k // 3, k // 3, k]):
            rowptr, col, val, shape = sr.permute_rows_cols(A, rows, np.arange(A.shape[1]), A.shape[1])
            h = eng.csr_select_rows(Ad.handle, rows, None if cuts is None else np.array(cuts, dtype=np.int32))
            _same_arrays(eng, h, rowptr, col, val, shape, "%s %s %s" % (source, what, cuts))
            broken = sr.plan_respects(h.row_blocks(), cuts, 0, None)
            assert broken is None, "%s %s %s: %s" % (source, what, cuts, broken)
            if k:
                _check_spmv(eng, h, rowptr, col, val, shape, "%s %s" % (source, what))


def test_bad_cuts_are_refused_and_the_engine_goes_on(hip_engine):
    from hipla.hip_engine import NssError
    eng = hip_engine
    A = cases.permute_sources()["ragged"]
    Ad = _upload(A)
    rows, ident = np.arange(20), np.arange(300)
    with pytest.raises(NssError, match="csr_permute: cuts must be ascending row positions"):
        eng.csr_permute(Ad.handle, rows, ident, 300, cuts=np.array([5, 3], dtype=np.int32))
    with pytest.raises(NssError, match="csr_permute: cuts must be ascending row positions"):
        eng.csr_permute(Ad.handle, rows, ident, 300, cuts=np.array([21], dtype=np.int32))
    with pytest.raises(NssError, match="csr_select_rows: cuts must be ascending row positions"):
        eng.csr_select_rows(Ad.handle, rows, cuts=np.array([-1], dtype=np.int32))
    with pytest.raises(ValueError, match="row index out of range"):
        eng.csr_permute(Ad.handle, np.array([300]), ident, 300)
    with pytest.raises(ValueError, match="column map out of range"):
        eng.csr_permute(Ad.handle, rows, ident, 299)
    h = eng.csr_permute(Ad.handle, rows, ident, 300, cuts=np.array([3, 5], dtype=np.int32))
    _same_arrays(eng, h, *sr.permute_rows_cols(A, rows, ident, 300))
