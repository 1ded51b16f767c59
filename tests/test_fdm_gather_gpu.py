"""The 1-D factors of the fast-diagonalisation solvers read off a resident matrix (csrc/fdm_gather.hip, DESIGN.md section
19): `hipla.fdm.gather_factors` against the extraction `hipla.fdm.fdm_factors` does on the host, on the operators of the
grid, on mutated copies of them, on a padded layout and on dense factors, and the refusals of the entry point.

Nothing here is a tolerance: a factor is gathered entries of the matrix less one fp64 product, the same operands in the
same operation on both sides, so the arrays must be EQUAL."""

import ctypes as C
import functools

import numpy as np
import pytest
import scipy.sparse as sp

pytestmark = pytest.mark.gpu

GRIDS = [(2, 3), (2, 5), (3, 3), (3, 4), (3, 9)]              # (3, 9): 1944 rows; its lines take 78 lanes
SEEDS = [0, 1, 2]
MUTATIONS = ["scaled", "dropped", "extra_inside", "extra_outside", "stored_zero", "nan", "on_line"]


@functools.lru_cache(maxsize=None)
def operators(dim, n):
    """(system, A, Lp) of the grid, computed once and never changed."""
    from staggered_grid import mac_stokes
    s = mac_stokes(dim, n, 0.01)
    A = sp.csr_matrix(s.A)
    A.sort_indices()
    Lp = (s.B @ (sp.diags(np.full(s.n_u, 1.0 / s.h ** s.dim)) @ s.B.T)).tocsr()
    Lp.sort_indices()
    return s, A, Lp


def layout(components, n_total):
    from hipla import fdm
    bases, pitch = fdm._affine_layout([np.asarray(g, dtype=np.int64) for g in components], n_total)
    return bases, pitch, [np.asarray(g).shape for g in components]


def host_rule(mat, components):
    """The extraction of `fdm_factors`, restated: per component the factors of its sub-matrix."""
    out = []
    for g in components:
        flat = np.asarray(g).reshape(-1)
        L = sp.csr_matrix(mat[flat][:, flat], dtype=np.float64, copy=True)
        L.eliminate_zeros()
        d, corner, T = g.ndim, L[0, 0], []
        for a, e in enumerate(g.shape):
            line = np.arange(e, dtype=np.int64) * int(np.prod(g.shape[a + 1:], dtype=np.int64))
            t = L[line][:, line].toarray()
            t[np.diag_indices(e)] -= (d - 1) / d * corner
            T.append(t)
        out.append(T)
    return out


def same(got, want):
    assert len(got) == len(want)
    for ts, ws in zip(got, want):
        assert len(ts) == len(ws)
        for t, w in zip(ts, ws):
            assert t.shape == w.shape and np.array_equal(t, w, equal_nan=True), (t, w)


def resident(mat):
    import hipla
    return hipla.SparseMatrix(mat.shape[0], mat.shape[1], mat.indptr, mat.indices, mat.data)


def mutate(mat, components, kind, seed):
    """A copy of `mat` (CSR, sorted) with one thing changed at a seeded place, or None where there is no room for it."""
    rng = np.random.default_rng(1000 * seed + len(kind))
    coo = sp.coo_matrix(mat)
    row, col, val = coo.row.copy(), coo.col.copy(), coo.data.copy()
    lab = np.full(mat.shape[0], -1)
    for c, g in enumerate(components):
        lab[np.asarray(g).reshape(-1)] = c
    at = int(rng.integers(len(val)))
    if kind == "on_line":                                     # an entry of a row on a line through a component's origin
        g = np.asarray(components[seed % len(components)])
        line = g[(slice(None),) + (0,) * (g.ndim - 1)] if seed % 2 else g[(0,) * (g.ndim - 1)]
        r = int(line[int(rng.integers(len(line)))])
        at = int(np.flatnonzero((row == r) & (col == r))[0])  # its diagonal: on every line through the point
    r = int(row[at])
    held = set(col[row == r].tolist())
    inside = [c for c in np.flatnonzero(lab == lab[r]) if c not in held]
    outside = [c for c in np.flatnonzero(lab != lab[r])]
    extra = None
    if kind in ("scaled", "on_line"):
        val[at] *= 1.0 + 1e-9
    elif kind == "dropped":
        row, col, val = (np.delete(x, at) for x in (row, col, val))
    elif kind == "nan":
        val[at] = np.nan
    elif kind == "extra_inside":
        extra = (inside, 1e-14 * abs(val).max())
    elif kind == "extra_outside":
        extra = (outside, 0.37)
    elif kind == "stored_zero":
        extra = (inside or outside, 0.0)
    if extra is not None:
        if not extra[0]:
            return None
        c = int(extra[0][int(rng.integers(len(extra[0])))])
        row, col, val = np.append(row, r), np.append(col, c), np.append(val, extra[1])
    order = np.lexsort((col, row))
    row, col, val = row[order], col[order], val[order]
    rowptr = np.concatenate([[0], np.cumsum(np.bincount(row, minlength=mat.shape[0]))])
    return sp.csr_matrix((val, col, rowptr), shape=mat.shape)


@pytest.mark.parametrize("dim,n", GRIDS)
def test_grid_operators_give_the_hosts_factors(hip_engine, dim, n):
    from hipla.fdm import fdm_factors, gather_factors, inverse_factors
    s, A, Lp = operators(dim, n)
    host, why = inverse_factors(A, s.component_ids)
    assert why is None
    got = gather_factors(resident(A), *layout(s.component_ids, A.shape[0]))
    same(got, [f.T for f in host.factors])
    extents = (s.n,) * s.dim
    host, why = fdm_factors(Lp, extents)
    assert why is None
    cells = [np.arange(s.n_p).reshape(extents)]
    same(gather_factors(resident(Lp), *layout(cells, s.n_p)), [host.T])


@pytest.mark.parametrize("dim,n", GRIDS)
def test_mutated_operators_give_the_factors_of_the_hosts_rule(hip_engine, dim, n):
    """One value scaled, one entry dropped, an extra entry inside the component and one in another component, a stored
    zero, a NaN, and a scaled entry of a row on a line through an origin: three seeded places each on A over the
    velocity components, the first seed on Lp over the cells."""
    from hipla.fdm import gather_factors
    s, A, Lp = operators(dim, n)
    cells = [np.arange(s.n_p).reshape((s.n,) * s.dim)]
    moved = 0
    for mat, components, seeds in ((A, s.component_ids, SEEDS), (Lp, cells, SEEDS[:1])):
        clean = host_rule(mat, components)
        for kind in MUTATIONS:
            for seed in seeds:
                bad = mutate(mat, components, kind, seed)
                if bad is None:
                    assert kind == "extra_outside" and mat is Lp       # one component: nothing outside it
                    continue
                want = host_rule(bad, components)
                same(gather_factors(resident(bad), *layout(components, mat.shape[0])), want)
                moved += any(not np.array_equal(t, w) for ts, ws in zip(want, clean) for t, w in zip(ts, ws))
    assert moved >= len(SEEDS) + 1                            # the "on_line" cases at the least change a factor


def test_padded_layout_and_dense_factors(hip_engine):
    """One component (3, 4, 5) at base 3 with pitch 29 in 85 rows (3 rows in front, 9 between the slabs, a tail of 4),
    its matrix the Kronecker sum of dense random symmetric factors: every T_a row holds e_a entries."""
    from hipla import fdm
    rng = np.random.default_rng(11)
    extents, base, pitch, n_total = (3, 4, 5), 3, 29, 3 + 2 * 29 + 20 + 4
    T = []
    for e in extents:
        t = rng.standard_normal((e, e))
        T.append(t + t.T + 3.0 * e * np.eye(e))
    K = sp.coo_matrix(fdm.kronecker_sum(T))
    assert K.nnz == 60 * (1 + 2 + 3 + 4)
    ids = base + np.arange(3)[:, None, None] * pitch + np.arange(4)[None, :, None] * 5 + np.arange(5)[None, None, :]
    flat = ids.reshape(-1)
    outside = np.setdiff1d(np.arange(n_total), flat)
    assert len(outside) == 25 and outside[0] == 0
    mat = sp.coo_matrix((np.concatenate([K.data, np.ones(len(outside))]),
                         (np.concatenate([flat[K.row], outside]), np.concatenate([flat[K.col], outside]))),
                        shape=(n_total, n_total)).tocsr()
    mat.sort_indices()
    assert layout([ids], n_total) == ([base], pitch, [extents])
    got = fdm.gather_factors(resident(mat), [base], pitch, [extents])
    same(got, host_rule(mat, [ids]))
    host, why = fdm.fdm_factors(mat[flat][:, flat].tocsr(), extents)
    assert why is None
    same(got, [host.T])
    dense = fdm.kronecker_sum(T)                              # the same factors without padding
    same(fdm.gather_factors(resident(dense), [0], 20, [extents]), [host.T])


def test_argument_errors_are_codes(hip_engine):
    """NULL pointers, counts out of range, layouts that fdm_layout.h refuses, a matrix of another size and a narrowed
    one: a code and a message each, and the next call works."""
    from hipla import fdm
    eng = hip_engine
    lib = eng.lib
    s, A, _ = operators(2, 5)
    dev = resident(A)
    bases, pitch, shapes = layout(s.component_ids, dev.m)
    assert (bases, pitch, shapes) == ([0, 4], 9, [(5, 4), (4, 5)])
    room = [np.zeros((e, e)) for sh in shapes for e in sh]

    def call(mat=dev.handle.ptr, ncomp=2, dim=2, n_total=dev.m, base=bases, pitch=pitch, shapes=shapes, out=room):
        b = None if base is None else (C.c_int64 * len(base))(*base)
        e = None if shapes is None else (C.c_int64 * (2 * len(shapes)))(*[x for sh in shapes for x in sh])
        f = None if out is None else (C.c_void_p * len(out))(*[None if t is None else t.ctypes.data for t in out])
        return lib.nss_fdm_gather_factors(mat, ncomp, dim, n_total, b, pitch, e, f, eng.stream)

    refusals = [(dict(mat=None), "NULL"), (dict(base=None), "NULL"), (dict(shapes=None), "NULL"),
                (dict(out=None), "NULL"), (dict(out=room[:3] + [None]), "NULL factor"),
                (dict(ncomp=0), "ncomp"), (dict(ncomp=4), "ncomp"), (dict(dim=1), "dim"), (dict(dim=4), "dim"),
                (dict(n_total=0), "n_total"), (dict(n_total=2 ** 31), "n_total"), (dict(n_total=dev.m + 1), "n_total x"),
                (dict(pitch=0), "pitch"), (dict(pitch=3), "pitch"), (dict(base=[0, 1]), "overlap"),
                (dict(base=[-1, bases[1]]), "fit"), (dict(shapes=[(0, 5), shapes[1]]), "extent")]
    for kwargs, word in refusals:
        assert call(**kwargs) != 0, kwargs
        text = lib.nss_last_error().decode()
        assert word in text and "fdm_gather_factors" in text, (kwargs, text)
    assert call() == 0
    lines = [np.moveaxis(np.asarray(g), a, 0)[(slice(None),) + (0,) * (g.ndim - 1)] for g in s.component_ids
             for a in range(g.ndim)]
    for raw, line in zip(room, lines):                        # what the entry point itself writes: the entries, as stored
        assert np.array_equal(raw, A[line][:, line].toarray())
    narrow = resident(A)
    eng.csr_narrow_f32(narrow.handle)
    assert call(mat=narrow.handle.ptr) != 0 and "fp32" in lib.nss_last_error().decode()
    with pytest.raises(ValueError, match="fp32"):
        fdm.gather_factors(narrow, bases, pitch, shapes)
    with pytest.raises(ValueError, match="SparseMatrix"):
        fdm.gather_factors(A, bases, pitch, shapes)
    with pytest.raises(ValueError, match="components"):
        fdm.gather_factors(dev, bases, pitch, [(5, 4)])
    same(fdm.gather_factors(dev, bases, pitch, shapes), host_rule(A, s.component_ids))
