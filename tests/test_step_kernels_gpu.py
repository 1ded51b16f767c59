"""The kernels of the device-resident time step (csrc/step.hip, csrc/flux.hip) and the device-started CG (`nss_cg_start`,
`CgLoop.solve_resident`) one at a time, through the C ABI as `hipla.fused.TimeStepper` calls it, on operands a
staggered grid never produces: random two-slot rows with 0, 1 or 2 entries (equal columns included), non-uniform
masses, the `done` flag, partial arrays on both sides of every change of shape of the summation tree.

References are numpy / scipy in fp64: row sums are formed in extended precision (`matvec`) and rounded once, every
total by `math.fsum`.  Tolerance: DESIGN.md section 3 and tests/test_hip_kernels.py -- 1e-13 for a kernel against numpy,
measured against the scale of the terms (|M||x| + |f| per row, sum |x_i| for a sum: at most 40 000 terms summed by a
tree at most 25 deep err by less than 25 * 2^-53 = 3e-15 of it) -- and bit equality where the code promises it.

What `SparseMatrix.from_scipy` cannot represent: a row whose single entry sits in the SECOND slot (the fixed-width copy
is filled from the CSR row, first slot first), so the `col = -1` first slot with a live second one is not reachable.
Not reached either: the grid-stride second trip of the one-lane-per-row kernels (more than 65 536 * 256 rows)."""

import ctypes as C
import itertools
from math import fsum, sqrt

import numpy as np
import pytest
import scipy.sparse as sp

from oracle import krylov_ref as kr

pytestmark = pytest.mark.gpu

TOL = 1e-13
SENT = -7.25                       # what output buffers hold before a launch
LD = np.longdouble
TAU = 0.05


def matvec(mat, x):
    """mat @ x with every row summed in extended precision (64-bit mantissa: a row of n entries errs by n * 2^-64 of
    |mat||x|), so that what is left after one rounding to fp64 is the reference's; `math.fsum` per row elsewhere."""
    mat = sp.csr_matrix(mat)
    x = np.asarray(x, dtype=np.float64)
    out = np.zeros(mat.shape[0], dtype=LD)
    if np.finfo(LD).eps > 2.0 ** -63:
        for r in range(mat.shape[0]):
            s, e = mat.indptr[r], mat.indptr[r + 1]
            out[r] = fsum(mat.data[s:e] * x[mat.indices[s:e]])
        return out
    prod = mat.data.astype(LD) * x[mat.indices].astype(LD)
    has = np.diff(mat.indptr) > 0
    if prod.size:
        out[has] = np.add.reduceat(prod, mat.indptr[:-1][has])
    return out


def absvec(mat, x):
    """|mat| |x|.  (Not through abs(mat): scipy sums the duplicate entries of a row first, in the arrays `mat` shares.)"""
    mat = sp.csr_matrix(mat)
    return np.asarray(matvec(sp.csr_matrix((np.abs(mat.data), mat.indices, mat.indptr), shape=mat.shape), np.abs(x)),
                      dtype=np.float64)


def two_slot(rng, m, n, counts=None):
    """Random (m, n) CSR with 0, 1 or 2 entries per row (a third of the rows each unless `counts` is given), random
    columns, every fourth two-entry row holding the SAME column twice (kept as two entries: no summing of duplicates)."""
    counts = rng.permutation(np.arange(m) % 3) if counts is None else np.asarray(counts)
    indptr = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    cols = rng.integers(0, n, size=int(indptr[-1])).astype(np.int32)
    twice = indptr[:-1][counts == 2][::4]
    cols[twice + 1] = cols[twice]
    mat = sp.csr_matrix((rng.standard_normal(cols.size), cols, indptr), shape=(m, n))
    mat.sort_indices()
    assert mat.nnz == cols.size
    return mat


def assert_every_count(mat):
    lens = np.diff(mat.indptr)
    assert lens.max() <= 2
    for k in (0, 1, 2):
        assert (lens == k).sum() >= 0.1 * mat.shape[0], (k, mat.shape)


def three_entry_row(rng, m, n):
    mat = two_slot(rng, m, n).tolil()
    mat[m // 2, :3] = [1.0, 2.0, 3.0]
    return mat.tocsr()


def upload(eng, mat, rows_form=False):
    """`rows_form`: created with the direct-rows threshold at 0, i.e. with the fixed-width copy and the row blocks of
    the row-per-lane kernel."""
    import hipla
    if not rows_form:
        return hipla.SparseMatrix.from_scipy(mat)
    with eng.overrides(direct_rows=0):
        return hipla.SparseMatrix.from_scipy(mat)


def flag(eng, value):
    return eng.torch.tensor([value], dtype=eng.torch.int32, device=eng.device)


def ptr(buf):
    return None if buf is None else buf.data_ptr()


def refused(eng, rc, word):
    msg = eng.lib.nss_last_error().decode()
    assert rc != 0 and word in msg, (rc, msg)


# ---- 1. nss_step_flux_f64 -----------------------------------------------------------------------------------------
def flux_case(eng, rng, nflux, n_u, counts=None):
    """One launch on random operators; returns the largest error in units of |adv||avg| + |adv||diff| / 2."""
    zero = nflux // 2
    if counts is None:                               # adv == 0.0 exactly beside live avg and diff: an empty adv row
        lens = [rng.permutation(np.arange(nflux) % 3) for _ in range(3)]
        for k, length in enumerate((0, 2, 1)):
            lens[k][zero] = length
    else:
        lens = [[c] for c in counts]
    adv, avg, dif = (two_slot(rng, nflux, n_u, k) for k in lens)
    if counts is None:
        for mat in (adv, avg, dif):
            assert_every_count(mat)
    u = rng.standard_normal(n_u)
    host = np.concatenate([u, np.full(nflux + 1, SENT)])          # [u | F | one guard entry]
    buf = eng.from_host(host)
    mats = [upload(eng, mat) for mat in (adv, avg, dif)]
    flux_ptr = buf.data_ptr() + 8 * n_u
    assert flux_ptr % 16 == 8                                     # n_u is odd: the segment starts on an odd element
    eng._check(eng.lib.nss_step_flux_f64(*(m.handle.ptr for m in mats), buf.data_ptr(), flux_ptr, None, eng.stream))
    got = eng.to_host(buf)
    assert np.array_equal(got[:n_u], u) and got[-1] == SENT
    a, m, d = matvec(adv, u), matvec(avg, u), matvec(dif, u)
    want = np.asarray(a * m - np.abs(a) * d / 2, dtype=np.float64)
    scale = absvec(adv, u) * absvec(avg, u) + absvec(adv, u) * absvec(dif, u) / 2
    err = np.abs(got[n_u:-1] - want)
    assert (err <= TOL * scale).all(), (np.nonzero(err > TOL * scale)[0][:8], err.max())
    if counts is None:
        a64 = np.asarray(a, dtype=np.float64)
        assert (a64 > 0).any() and (a64 < 0).any() and a64[zero] == 0.0 and got[n_u + zero] == 0.0
        central = np.asarray(a * m, dtype=np.float64)             # without the upwind term
        assert np.linalg.norm(central - want) > 1e-6 * np.linalg.norm(want)
    return float(np.max(err[scale > 0] / scale[scale > 0])) if (scale > 0).any() else 0.0


@pytest.mark.parametrize("n_u", [7, 1001])
@pytest.mark.parametrize("nflux", [1, 255, 256, 257, 1000])
def test_flux_on_random_two_slot_operators(hip_engine, nflux, n_u):
    """F = adv * avg - |adv| diff / 2 to 1e-13 per row, u untouched, the upwind term visible, adv == 0.0 exactly in a
    row whose avg and diff are live.  One flux point: every (adv, avg, diff) row length that a row can take."""
    rng = np.random.default_rng(1000 * nflux + n_u)
    if nflux == 1:
        errs = [flux_case(hip_engine, rng, 1, n_u, counts) for counts in itertools.product((0, 1, 2), repeat=3)]
    else:
        errs = [flux_case(hip_engine, rng, nflux, n_u)]
    print("flux nflux=%d n_u=%d max err / scale = %.3e" % (nflux, n_u, max(errs)))


def test_flux_refusals_and_no_flux_points(hip_engine):
    eng, lib = hip_engine, hip_engine.lib
    rng = np.random.default_rng(5)
    n_u = 33
    good = [upload(eng, two_slot(rng, 40, n_u)) for _ in range(3)]
    wide = upload(eng, three_entry_row(rng, 40, n_u))
    buf = eng.from_host(np.concatenate([rng.standard_normal(n_u), np.full(41, SENT)]))
    before = eng.to_host(buf).copy()
    tail = buf.data_ptr() + 8 * n_u
    for pos in range(3):
        mats = list(good)
        mats[pos] = wide
        refused(eng, lib.nss_step_flux_f64(*(m.handle.ptr for m in mats), buf.data_ptr(), tail, None, eng.stream),
                "step_flux")
    bare = [upload(eng, sp.csr_matrix((3, 0))) for _ in range(3)]        # rows but no columns: u has no element 0
    refused(eng, lib.nss_step_flux_f64(*(m.handle.ptr for m in bare), buf.data_ptr(), tail, None, eng.stream),
            "no columns")
    empty = [upload(eng, sp.csr_matrix((0, n_u))) for _ in range(3)]
    assert lib.nss_step_flux_f64(*(m.handle.ptr for m in empty), buf.data_ptr(), tail, None, eng.stream) == 0, \
        lib.nss_last_error()
    assert np.array_equal(eng.to_host(buf), before)


# ---- 2. nss_step_rhs_f64 ------------------------------------------------------------------------------------------
def ragged(rng, m, extra=2600):
    """(m, m + extra): rows of 0 .. 8 entries, every seventh row empty, one row longer than an LDS chunk of 2048 (two
    where there is room) -- the shapes of test_spmv_ragged_empty_and_long_rows."""
    n = m + extra
    lens = rng.integers(0, 9, size=m)
    lens[::7] = 0
    lens[min(100, m - 1)] = 2500
    if m > 2999:
        lens[2999] = 4099
    rows = np.repeat(np.arange(m), lens)
    cols = np.concatenate([rng.choice(n, size=k, replace=False) for k in lens])
    return sp.csr_matrix((rng.standard_normal(rows.size), (rows, cols)), shape=(m, n))


def grid_ad(s):
    ad = sp.hstack([s.A, s.convection_operators()["div"]], format="csr")
    ad.sort_indices()
    return ad


@pytest.mark.parametrize("case", ["mac2d-7", "mac3d-4-inflated-3", "ragged-1", "ragged-257", "ragged-3000"])
def test_rhs_behind_every_branch_of_the_stream_kernel(hip_engine, case):
    """temp = f - [A | D] [u | F] to 1e-13 of |M||uf| + |f| per row: grid operators (staged operand), their inflated
    form (grouped columns) and a ragged matrix (gathered operand, empty rows, rows reduced by the whole workgroup)."""
    from staggered_grid import mac_stokes
    eng = hip_engine
    rng = np.random.default_rng(len(case))
    if case.startswith("ragged"):
        mat = ragged(rng, int(case.split("-")[1]))
        assert np.diff(mat.indptr).max() > 2048
    else:
        mat = grid_ad(mac_stokes(2, 7) if case == "mac2d-7" else mac_stokes(3, 4).inflate(3))
    m, n = mat.shape
    uf, f = rng.standard_normal(n), rng.standard_normal(m)
    M = upload(eng, mat)
    d_uf, d_f, temp = eng.from_host(uf), eng.from_host(f), eng.from_host(np.full(m + 1, SENT))
    eng._check(eng.lib.nss_step_rhs_f64(M.handle.ptr, ptr(d_uf), ptr(d_f), ptr(temp), None, eng.stream))
    got = eng.to_host(temp)
    want = np.asarray(f - matvec(mat, uf), dtype=np.float64)
    scale = absvec(mat, uf) + np.abs(f)
    err = np.abs(got[:m] - want) / scale
    print("rhs %s %s form=%s max err / scale = %.3e" % (case, mat.shape, M.handle.info()["operand_form"], err.max()))
    assert got[m] == SENT
    assert np.array_equal(eng.to_host(d_uf), uf) and np.array_equal(eng.to_host(d_f), f)
    assert err.max() < TOL
    if m <= n:                                    # (temp as long as the operand it would alias)
        refused(eng, eng.lib.nss_step_rhs_f64(M.handle.ptr, ptr(d_uf), ptr(d_f), ptr(d_uf), None, eng.stream), "step_rhs")
    refused(eng, eng.lib.nss_step_rhs_f64(M.handle.ptr, ptr(d_uf), ptr(d_f), ptr(d_f), None, eng.stream), "step_rhs")


# ---- 3. nss_step_project_f64 --------------------------------------------------------------------------------------
PROJECT_ROWS = (1, 255, 256, 257, 511, 512, 513, 2048, 4097)      # 2048: exactly 8 row blocks of 256 rows


def project_operands(m, n_p):
    """The generator of a case and its C (None for one row: the caller takes every row length).  The masses
    0.5 + random have mean 1, so the weighted and the unweighted energy differ by O(m^-1/2) only: with these seeds by
    more than 2.7e-3 in every case (checked on the host with the reference fields), which the tests assert as 1e-3."""
    rng = np.random.default_rng(11 * m + n_p)
    if m == 1:
        return rng, None
    c = two_slot(rng, m, n_p)
    assert_every_count(c)
    return rng, c


def project_launch(eng, Cm, dev, use_u, use_mass, use_part, in_place, done=None):
    """Fresh device copies of the operands in `dev` (host arrays), one launch; returns (out, u, partials) on the host."""
    phi, raw = eng.from_host(dev["phi"]), eng.from_host(dev["raw"])
    out = raw if in_place else eng.from_host(np.full(dev["raw"].size, SENT))
    u = eng.from_host(dev["u0"]) if use_u else None
    mass = eng.from_host(dev["mass"]) if use_mass else None
    part = eng.from_host(np.full(dev["nblk"] + 5, SENT)) if use_part else None
    eng._check(eng.lib.nss_step_project_f64(Cm.handle.ptr, ptr(phi), ptr(raw), ptr(out), ptr(u), TAU, ptr(mass),
                                            ptr(part), dev["nblk"] + 5, ptr(done), eng.stream))
    assert np.array_equal(eng.to_host(phi), dev["phi"])
    if not in_place:
        assert np.array_equal(eng.to_host(raw), dev["raw"])
    return eng.to_host(out), None if u is None else eng.to_host(u), None if part is None else eng.to_host(part)


def project_check(eng, c, mass, rng, combos, tag):
    """Both plans of `c`, the call combinations `combos` = (u, mass, partials, in place) on each; returns the plans'
    row-block counts."""
    m, n_p = c.shape
    host = dict(phi=rng.standard_normal(n_p), raw=rng.standard_normal(m), u0=rng.standard_normal(m), mass=mass)
    cphi = matvec(c, host["phi"])
    want_out = np.asarray(host["raw"] - cphi, dtype=np.float64)
    scale_out = np.abs(host["raw"]) + absvec(c, host["phi"])
    want_u = np.asarray(host["u0"] + TAU * (host["raw"] - cphi), dtype=np.float64)
    scale_u = np.abs(host["u0"]) + TAU * scale_out
    results, blocks, worst = {}, {}, dict(out=0.0, u=0.0, energy=0.0)
    for plan in ("stream", "rows"):
        Cm = upload(eng, c, rows_form=plan == "rows")
        if c.nnz:
            assert (Cm.handle.info()["operand_form"] == "rows") == (plan == "rows")
        rb = Cm.handle.row_blocks()
        blocks[plan] = (len(rb) - 1, int(np.diff(rb).max()))
        host["nblk"] = len(rb) - 1
        for combo in combos:
            use_u, use_mass, use_part, in_place = combo
            out, u, part = project_launch(eng, Cm, host, *combo)
            results[(plan,) + combo] = (out, u)
            worst["out"] = max(worst["out"], np.max(np.abs(out - want_out) / scale_out))
            if use_u:
                worst["u"] = max(worst["u"], np.max(np.abs(u - want_u) / scale_u))
            if use_part:
                e = u if use_u else out                           # the device's own field: the check is of the sum
                weighted = fsum((mass if use_mass else 1.0) * e * e)
                err = abs(fsum(part[:host["nblk"]]) - weighted) / weighted
                worst["energy"] = max(worst["energy"], err)
                assert (part[host["nblk"]:] == SENT).all() and (part[:host["nblk"]] >= 0.0).all()
                if use_mass:                                      # the weight is visible
                    assert abs(fsum(e * e) - weighted) > 1e-3 * weighted, (fsum(e * e), weighted)
    for combo in combos:
        for a, b in zip(results[("stream",) + combo], results[("rows",) + combo]):
            assert (a is None and b is None) or np.array_equal(a, b), combo
    print("project %s m=%d n_p=%d blocks (count, longest) %s max err / scale: out %.3e u %.3e energy %.3e"
          % (tag, m, n_p, blocks, worst["out"], worst["u"], worst["energy"]))
    assert worst["out"] < TOL and worst["u"] < TOL and worst["energy"] < TOL
    return blocks


ALL_CALLS = tuple(itertools.product((False, True), repeat=4))


@pytest.mark.parametrize("n_p", [1, 300])
@pytest.mark.parametrize("m", PROJECT_ROWS)
def test_project_every_call_form_on_both_plans(hip_engine, m, n_p):
    """out = raw - C phi, u = u0 + tau out and the row-block partials of sum m_r e_r^2 to 1e-13 for every combination
    of u / mass / partials / in place, on the plan of a small matrix and on the row-per-lane plan, bit-identical
    between the two; partials behind the row blocks keep their sentinel; the mass weight is visible."""
    rng, c = project_operands(m, n_p)
    mass = 0.5 + rng.random(m)
    if c is not None:
        project_check(hip_engine, c, mass, rng, ALL_CALLS, "random")
        return
    for count in (0, 1, 2):                                       # one row: every length it can take
        project_check(hip_engine, two_slot(rng, 1, n_p, [count]), mass, rng, ALL_CALLS, "one row of %d" % count)


def test_project_row_block_shapes(hip_engine):
    """The row-block counts of the cases above cover a grid without padding workgroups (8), grids that are mostly
    padding (fewer than 8) and a grid with a padded tail (more than 8, no multiple of 8).  At these sizes both plans
    cut blocks of at most 256 rows (the plan of a small matrix prefers many short row blocks), so the `base` loop of
    the row-per-lane kernel makes one trip; a matrix of 3 * 256 * 2048 + 77 rows keeps 768-row blocks under the
    stream plan -- two trips, the second one half full -- and 512-row blocks under the row-per-lane plan."""
    eng = hip_engine
    counts = set()
    for m in PROJECT_ROWS[1:]:
        c = project_operands(m, 300)[1]
        for rows_form in (False, True):
            counts.add(len(upload(eng, c, rows_form).handle.row_blocks()) - 1)
    assert any(k < 8 for k in counts) and 8 in counts and any(k > 8 and k % 8 for k in counts), counts
    m, n_p = 3 * 256 * 2048 + 77, 300
    rng = np.random.default_rng(3)
    c = two_slot(rng, m, n_p)
    assert_every_count(c)
    mass = 0.5 + rng.random(m) ** 2
    calls = ((True, True, True, False), (False, False, True, True))
    blocks = project_check(eng, c, mass, rng, calls, "long blocks")
    assert 512 < blocks["stream"][1] <= 1024 and blocks["rows"][1] == 512, blocks
    assert blocks["stream"][0] % 8 and blocks["rows"][0] % 8


def test_project_refusals(hip_engine):
    eng, lib = hip_engine, hip_engine.lib
    rng = np.random.default_rng(9)
    m, n_p = 700, 50
    Cm = upload(eng, two_slot(rng, m, n_p))
    nblk = len(Cm.handle.row_blocks()) - 1
    assert nblk > 1
    phi, raw, out, u = (eng.from_host(rng.standard_normal(k)) for k in (n_p, m, m, m))
    part = eng.from_host(np.full(nblk, SENT))

    def call(mat, out_, u_, part_, cap):
        return lib.nss_step_project_f64(mat.handle.ptr, ptr(phi), ptr(raw), ptr(out_), ptr(u_), TAU, None, ptr(part_), cap,
                                        None, eng.stream)
    refused(eng, call(Cm, out, u, part, nblk - 1), "step_project")
    refused(eng, call(Cm, out, out, None, 0), "step_project")
    refused(eng, call(Cm, out, raw, None, 0), "step_project")
    refused(eng, call(upload(eng, three_entry_row(rng, m, n_p)), out, u, None, 0), "step_project")
    assert call(Cm, out, u, None, 0) == 0 and call(Cm, out, u, part, nblk) == 0      # ... and what is in order runs
    assert call(upload(eng, sp.csr_matrix((0, n_p))), out, u, None, 0) == 0, lib.nss_last_error()
    assert (eng.to_host(part) >= 0.0).all()


# ---- 4. nss_step_divergence_f64, nss_step_workspace, nss_step_record_f64 -------------------------------------------
def workspace(eng, Cm, Bm):
    ne, nd = C.c_int64(), C.c_int64()
    eng._check(eng.lib.nss_step_workspace(Cm.handle.ptr, Bm.handle.ptr, C.byref(ne), C.byref(nd)))
    return ne.value, nd.value


def random_b(rng, m, n=700):
    lens = rng.integers(1, 41, size=m)
    if m > 4:
        lens[::5] = 0
        lens[3] = 40
    rows = np.repeat(np.arange(m), lens)
    cols = np.concatenate([rng.choice(n, size=k, replace=False) for k in lens] + [np.zeros(0, dtype=np.int64)])
    return sp.csr_matrix((rng.standard_normal(rows.size), (rows, cols)), shape=(m, n))


@pytest.mark.parametrize("m", [1, 256, 257, 5000])
def test_divergence_partials(hip_engine, m):
    """sqrt(sum of the partials) = |B u| to 1e-13 of the norm of |B||u|; the count of nss_step_workspace is the number
    of partials written, one entry less is refused.  Rows of 0 .. 40 entries, every fifth one empty."""
    eng = hip_engine
    rng = np.random.default_rng(40 + m)
    b = random_b(rng, m)
    assert b.nnz and (m == 1 or (np.diff(b.indptr) == 0).any()) and np.diff(b.indptr).max() <= 40
    Bm = upload(eng, b)
    Cm = upload(eng, two_slot(rng, 300, 20))
    ne, nd = workspace(eng, Cm, Bm)
    assert ne == len(Cm.handle.row_blocks()) - 1 and nd == (m + 255) // 256
    u = rng.standard_normal(b.shape[1])
    d_u, part = eng.from_host(u), eng.from_host(np.full(nd + 4, SENT))
    refused(eng, eng.lib.nss_step_divergence_f64(Bm.handle.ptr, ptr(d_u), ptr(part), nd - 1, None, eng.stream),
            "step_divergence")
    assert (eng.to_host(part) == SENT).all()
    eng._check(eng.lib.nss_step_divergence_f64(Bm.handle.ptr, ptr(d_u), ptr(part), nd + 4, None, eng.stream))
    got = eng.to_host(part)
    assert (got[:nd] >= 0.0).all() and (got[nd:] == SENT).all()
    bu = matvec(b, u)
    want = sqrt(fsum(np.asarray(bu * bu, dtype=np.float64)))
    scale = sqrt(fsum(absvec(b, u) ** 2))
    err = abs(sqrt(fsum(got[:nd])) - want)
    print("divergence m=%d partials=%d |Bu|=%.6e err / |Bu| = %.3e err / scale = %.3e"
          % (m, nd, want, err / want if want else 0.0, err / scale if scale else 0.0))
    assert err <= TOL * scale


SUM_LENGTHS = (0, 1, 63, 64, 65, 1023, 1024, 1025, 4095, 4096, 4097, 8193, 35000)
SUM_PAIRS = tuple((n, n) for n in SUM_LENGTHS) + ((4096, 4097), (4097, 0), (1, 35000))


def record(eng, pk, pd, scale, slot=3, slots=5, done=None, n_d=None):
    """One nss_step_record_f64 launch into a record of `slots` sentinel pairs; host arrays in, the record out.  An empty
    array is passed as a live pointer with length 0; `n_d` overrides the length given for `pd`."""
    d_pk = eng.from_host(pk if pk.size else np.full(1, SENT))
    d_pd = None if pd is None else eng.from_host(pd if pd.size else np.full(1, SENT))
    if n_d is None:
        n_d = 7 if pd is None else pd.size                        # (without pd the length is not looked at)
    rec = eng.from_host(np.full(2 * slots, SENT))
    eng._check(eng.lib.nss_step_record_f64(ptr(d_pk), pk.size, ptr(d_pd), n_d, scale, ptr(rec), slot, ptr(done), eng.stream))
    return eng.to_host(rec)


@pytest.mark.parametrize("na,nb", SUM_PAIRS)
def test_record_sums_arbitrary_partials(hip_engine, na, nb):
    """The one entry point that exposes `fixed_sums_1024` without a solver around it, on signed N(0, 1) terms:
    record[2 slot] = scale * sum pk to 1e-13 * scale * sum |pk|; record[2 slot + 1]^2 = sum pd to 1e-13 * sum |pd|
    (pd is negated as a whole where its sum is negative: the kernel takes the root of the sum, not of its modulus) and
    the root itself on non-negative terms; both totals BIT FOR BIT the oracle's restatement of the loop formulation,
    on both sides of the 4096 terms at which the device code changes formulation.  A length of 0 is accepted (the
    header asks for no minimum): the total is 0.0."""
    eng = hip_engine
    rng = np.random.default_rng(10000 * na + nb)
    pk, pd = rng.standard_normal(na), rng.standard_normal(nb)
    if fsum(pd) < 0.0:
        pd = -pd
    scale = 0.37
    rec = record(eng, pk, pd, scale)
    other = np.delete(np.arange(10), [6, 7])
    assert (rec[other] == SENT).all()
    err_k = abs(rec[6] - scale * fsum(pk))
    err_d = abs(rec[7] * rec[7] - fsum(pd))
    abs_k, abs_d = fsum(np.abs(pk)), fsum(np.abs(pd))
    assert err_k <= TOL * scale * abs_k and err_d <= TOL * abs_d
    pos = np.abs(pd)
    root = record(eng, pk, pos, scale)
    err_r = abs(root[7] - sqrt(fsum(pos)))
    assert err_r <= TOL * sqrt(fsum(pos)) and root[6] == rec[6]
    print("record (%d, %d) err / (scale sum|pk|) = %.3e, err of square / sum|pd| = %.3e, err of root / root = %.3e"
          % (na, nb, err_k / (scale * abs_k) if na else 0.0, err_d / abs_d if nb else 0.0,
             err_r / sqrt(fsum(pos)) if nb else 0.0))
    bare = record(eng, pk, None, scale)                            # without pd: NaN, and the same first entry
    assert np.isnan(bare[7]) and bare[6] == rec[6] and (bare[other] == SENT).all()
    assert all(np.array_equal(record(eng, pk, pd, scale), rec) for _ in range(5))
    # the tree, bit for bit.  Scale 1.0: the first entry is pk's total itself.  pd's total is only seen through the
    # device's square root (specified to 1 ulp, numpy's is correctly rounded): one spacing is allowed there, and the same
    # array is summed on the other side, where the total shows, in a second launch.
    exact = record(eng, pk, pd, 1.0)
    sa, sb = kr.fixed_sums_1024(pk, pd)
    assert exact[6] == sa, (na, exact[6], sa)
    assert abs(exact[7] - np.sqrt(sb)) <= np.spacing(np.sqrt(sb)), (nb, exact[7], np.sqrt(sb))
    swapped = record(eng, pd, pk, 1.0, n_d=0)                      # (pk: a live pointer given length 0)
    assert swapped[6] == sb and swapped[7] == 0.0


# ---- 5. the done flag ---------------------------------------------------------------------------------------------
def test_done_flag_of_every_step_launch(hip_engine):
    """A device int32 holding 1 turns each of the six launches into a no-op (every output buffer bit-unchanged); the
    same buffer holding 0 gives the bits of done = NULL."""
    eng, lib = hip_engine, hip_engine.lib
    rng = np.random.default_rng(77)
    n_u, nflux, n_p = 601, 900, 130
    adv, avg, dif = (upload(eng, two_slot(rng, nflux, n_u)) for _ in range(3))
    ad = upload(eng, sp.random(n_u, n_u + nflux, density=0.01, random_state=3, format="csr"))
    c_host = two_slot(rng, n_u, n_p)
    Cm = upload(eng, c_host)
    b_host = random_b(rng, n_p, n_u)
    Bm = upload(eng, b_host)
    ne, nd = workspace(eng, Cm, Bm)
    assert ne > 1
    host = dict(uf=np.concatenate([rng.standard_normal(n_u), np.full(nflux, SENT)]), f=rng.standard_normal(n_u),
                phi=rng.standard_normal(n_p), raw=rng.standard_normal(n_u), u0=rng.standard_normal(n_u),
                mass=0.5 + rng.random(n_u), pk=rng.standard_normal(3000), pd=rng.random(5000))

    def run(done):
        d = {k: eng.from_host(v) for k, v in host.items()}
        o = {k: eng.from_host(np.full(n, SENT)) for k, n in (("temp", n_u), ("out", n_u), ("part_e", ne), ("part_d", nd),
                                                             ("rec", 10))}
        dp = ptr(done)
        eng._check(lib.nss_step_flux_f64(adv.handle.ptr, avg.handle.ptr, dif.handle.ptr, ptr(d["uf"]),
                                         d["uf"].data_ptr() + 8 * n_u, dp, eng.stream))
        eng._check(lib.nss_step_rhs_f64(ad.handle.ptr, ptr(d["uf"]), ptr(d["f"]), ptr(o["temp"]), dp, eng.stream))
        eng._check(lib.nss_step_project_f64(Cm.handle.ptr, ptr(d["phi"]), ptr(d["raw"]), ptr(o["out"]), ptr(d["u0"]), TAU,
                                            ptr(d["mass"]), ptr(o["part_e"]), ne, dp, eng.stream))
        eng._check(lib.nss_step_divergence_f64(Bm.handle.ptr, ptr(d["u0"]), ptr(o["part_d"]), nd, dp, eng.stream))
        eng._check(lib.nss_step_record_f64(ptr(d["pk"]), 3000, ptr(d["pd"]), 5000, 0.5, ptr(o["rec"]), 2, dp, eng.stream))
        got = {k: eng.to_host(v) for k, v in o.items()}
        got["uf"], got["u"] = eng.to_host(d["uf"]), eng.to_host(d["u0"])
        return got

    stopped, zero, none = run(flag(eng, 1)), run(flag(eng, 0)), run(None)
    for key in ("temp", "out", "part_e", "part_d", "rec"):
        assert (stopped[key] == SENT).all(), key
    assert np.array_equal(stopped["uf"], host["uf"]) and np.array_equal(stopped["u"], host["u0"])
    for key, val in none.items():
        assert np.array_equal(zero[key], val), key
    assert not (none["temp"] == SENT).any() and not (none["uf"] == SENT).any() and not (none["out"] == SENT).any()
    assert (none["part_e"] >= 0).all() and (none["part_d"] >= 0).all() and (none["rec"][[4, 5]] != SENT).all()
    assert not np.array_equal(none["u"], host["u0"])


# ---- 6. nss_cg_start / CgLoop.solve_resident -----------------------------------------------------------------------
def tridiagonal(n):
    """SPD, condition number below 10, n distinct eigenvalues."""
    return sp.diags([-1.0, 2.5, -1.0], [-1, 0, 1], shape=(n, n), format="csr") if n > 1 else sp.csr_matrix([[2.5]])


CG_CASES = [("mac", pre) for pre in ("none", "jacobi", "bjac", "bgs", "amg")] + \
           [(size, pre) for size in ("tri1", "tri257") for pre in ("none", "jacobi")]


@pytest.mark.parametrize("system,pre_name", CG_CASES)
def test_cg_started_on_the_device(hip_engine, system, pre_name):
    """One `CgLoop` per preconditioner through: `solve`; `solve_resident` with the same right-hand side into an x of
    7.0 (count within one of `solve`'s -- the two starts sum <r, z> by different trees --, history and err0 to 1e-8,
    x against a direct solve to 1e-8); again with another right-hand side while the control word still says DONE;
    a zero right-hand side (0 iterations, x exactly 0); maxsteps = 3 (returns 3 -- the 1 x 1 system is solved by its
    first iteration and returns 1); maxsteps beyond the history's length (it grows; count and x as before, bit for
    bit).  Block Jacobi, Gauss-Seidel and the V-cycle are launches of their own (`cg_start_direction_kernel`)."""
    import hipla
    import scipy.sparse.linalg as spl
    from hipla import fused
    from hipla.hip_engine import NssError
    from staggered_grid import mac_stokes
    eng = hip_engine
    if system == "mac":
        s = mac_stokes(3, 6, 0.01)
        mat = s.A
    else:
        mat = tridiagonal(int(system[3:]))
    n = mat.shape[0]
    A = hipla.SparseMatrix.from_scipy(mat)
    pre = {"none": lambda: None, "jacobi": lambda: hipla.JacobiPreconditioner(A),
           "bjac": lambda: hipla.BlockJacobi(A, s.line_blocks(3)), "bgs": lambda: hipla.BlockGaussSeidel(A, s.line_blocks(3)),
           "amg": lambda: hipla.SmoothedAggregationAMG(A, coarse_size=60)}[pre_name]()
    loop = fused.CgLoop.try_create(A, pre)
    assert loop is not None, fused.CgLoop.last_declined
    rng = np.random.default_rng(31)
    b1, b2 = rng.standard_normal(n), rng.standard_normal(n)
    solve = spl.splu(sp.csc_matrix(mat)).solve
    d_b1, d_b2 = eng.from_host(b1), eng.from_host(b2)

    def sevens():
        return eng.from_host(np.full(n, 7.0))

    def against(x, b):
        exact = solve(b)
        return np.linalg.norm(eng.to_host(x) - exact) / np.linalg.norm(exact)

    x1 = sevens()
    it1, errs1 = loop.solve(d_b1, x1, 1e-10, 2000)                                      # 1
    x2 = sevens()
    it2 = loop.solve_resident(d_b1, x2, 1e-10, 2000)                                    # 2
    hist = eng.to_host(loop.hist)[:it2].copy()
    err0 = float(eng.to_host(loop.scal)[3])
    assert int(eng.to_host(loop.ctrl)[0]) == 1
    x3 = sevens()
    it3 = loop.solve_resident(d_b2, x3, 1e-10, 2000)                                    # 3: started with DONE = 1
    e2, e3 = against(x2, b1), against(x3, b2)
    print("cg %s/%s n=%d counts solve %d resident %d other rhs %d; x against direct solve %.3e %.3e"
          % (system, pre_name, n, it1, it2, it3, e2, e3))
    assert abs(it2 - it1) <= 1 and 0 < it2 < 2000 and 0 < it3 < 2000
    m = min(25, it1, it2)
    np.testing.assert_allclose(hist[:m], errs1[1:1 + m], rtol=1e-8)
    np.testing.assert_allclose(err0, errs1[0], rtol=1e-8)
    assert e2 < 1e-8 and e3 < 1e-8
    x4 = sevens()
    assert loop.solve_resident(eng.zeros(n), x4, 1e-10, 2000) == 0                      # 4
    assert (eng.to_host(x4) == 0.0).all()
    x5 = sevens()
    assert loop.solve_resident(d_b1, x5, 1e-10, 3) == (3 if n > 1 else 1)               # 5
    assert it1 > 3 or n == 1
    assert np.isfinite(eng.to_host(x5)).all() and loop.hist.numel() < 5000
    x6 = sevens()
    assert loop.solve_resident(d_b1, x6, 1e-10, 5000) == it2 and loop.hist.numel() >= 5000      # 6: the history grows
    assert np.array_equal(eng.to_host(x6), eng.to_host(x2))
    np.testing.assert_array_equal(eng.to_host(loop.hist)[:it2], hist)
    if pre_name in ("none", "jacobi"):
        _, ref_hist = kr.cg(mat, b1, pre=kr.jacobi(mat) if pre_name == "jacobi" else None, tol=1e-10, maxsteps=2000)
        assert abs(it2 - (len(ref_hist) - 1)) <= 1, (it2, len(ref_hist) - 1)
    with pytest.raises(NssError, match="cg_start"):
        loop.solve_resident(x6, x6, 1e-10, 10)
