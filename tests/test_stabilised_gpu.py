"""Stabilised saddle-point systems [[A, B^T], [B, C]] in the fused textbook BPCG and MINRES loops (csrc/bpcg1.hip,
csrc/minres.hip: one launch stores C x_p, the epilogue of B's rows adds it).

* The entry points against the goldens of the reference's own files, with the device loop counted.
* One iteration of the textbook BPCG (nss_bpcg1_phases) and two of MINRES (the second runs the scaled operand) from the
  methods' own start states against a numpy restatement of the reference's statements: every vector the iteration
  writes to 1e-13 of its max-abs (the project's SpMV parity bound), under every setting that changes which kernel B's
  rows and the sums take -- and all settings agree bit for bit.
* A stored zero C gives the bits of C = None; warm starts; nothing is written after the stop."""

import contextlib
import ctypes
import functools

import numpy as np
import pytest
import scipy.sparse as sp

import stabilised_cases as sc
from staggered_grid import mac_stokes

pytestmark = pytest.mark.gpu

BOUND = 1e-13


@contextlib.contextmanager
def fused_loops_counted():
    """Counts the runs of the two device-resident loops that take a C."""
    from hipla import fused
    counts = {"bpcg1": 0, "minres": 0}
    saved = {}
    for key, cls in (("bpcg1", fused.Bpcg1Loop), ("minres", fused.MinresLoop)):
        saved[cls] = cls.run

        def counting(self, *a, _key=key, _orig=cls.run, **kw):
            counts[_key] += 1
            return _orig(self, *a, **kw)
        cls.run = counting
    try:
        yield counts
    finally:
        for cls, orig in saved.items():
            cls.run = orig


@contextlib.contextmanager
def protocol_path():
    from hipla import fused
    fused.ENABLED = False
    try:
        yield
    finally:
        fused.ENABLED = True


# ---- the entry points against the goldens ----------------------------------------------------------------------------
@pytest.mark.parametrize("name", sc.NAMES)
def test_entry_points_match_the_goldens_in_the_device_loop(hip_engine, name):
    d = sc.load(name)
    case = sc.StabCase(d)
    with fused_loops_counted() as counts:
        sc.run_entry_point(d, case, sc.device_operands(case))
    assert counts[str(d["solver"])] == 1, "the fused device loop did not run: %r" % (counts,)


# ---- one iteration against numpy -------------------------------------------------------------------------------------
SIZES = [(2, 2), (2, 17), (3, 6)]      # n_p = 4; n_p = 289, n_u = 544 (tails in every block size); 3-D
C_KINDS = ("generator", "gram")


@functools.lru_cache(maxsize=None)
def system(dim, n, kind):
    """(StokesSystem, C, f, g, dinv, k): C from the generator, or C = -G G^T from a seeded sparse G with one zero row
    (an empty row and column of C) and one full row (a row of C with an entry at every non-empty row of G: more than
    a wavefront where n_p allows).  k = 1 / lambda_min(dinv A) + 1e-3 by a dense eigensolve."""
    s = mac_stokes(dim, n, 0.01)
    n_p = s.n_p
    if kind == "generator":
        C = s.pressure_stabilisation(1.0)
    else:
        rng = np.random.default_rng(5)
        G = sp.random(n_p, n_p, density=min(1.0, 3.0 / n_p), random_state=rng, format="lil")
        G[0, :] = 0.0
        G[1, :] = rng.standard_normal(n_p)
        G[2, 2] = 1.0
        G = sp.csr_matrix(G)
        G.eliminate_zeros()
        C = (-(G @ G.T)).tocsr() * (s.h ** dim)
        C.sort_indices()
        lens = np.diff(C.indptr)
        assert lens[0] == 0 and C[:, 0].nnz == 0
        assert lens[1] == np.count_nonzero(np.diff(G.indptr)) and (lens[1] > 64 or n_p < 80)
    f = s.rhs(0)[0]
    g = np.random.default_rng(1).standard_normal(n_p)
    g -= g.mean()
    dinv = 1.0 / s.A.diagonal()
    root = np.sqrt(dinv)
    lam = np.linalg.eigvalsh(root[:, None] * s.A.toarray() * root[None, :])
    return s, C, f, g, dinv, 1.0 / lam.min() + 1e-3


def worst(got, want):
    return max(float(np.abs(got[key] - want[key]).max() / np.abs(want[key]).max()) for key in want)


def bpcg1_start(dim, n, kind):
    """The state bramble_pasciak_cg.py:98-105 leaves in front of its loop, from a small non-zero start vector."""
    s, C, f, g, dinv, k = system(dim, n, kind)
    A, B, minv = s.A, s.B, 1.0 / s.mass
    rng = np.random.default_rng(3)
    xu, xp = 0.1 * rng.standard_normal(s.n_u), 0.1 * rng.standard_normal(s.n_p)
    Ku, Kp = A @ xu + B.T @ xp, B @ xu + C @ xp
    au, ap = k * dinv * (f - Ku), g - Kp                                     # :98-99
    ru, rp = A @ au - f + Ku, B @ au - g + Kp                                # :100-101
    t1u, t1p = au.copy(), minv * (B @ au - ap)                               # :102
    rho = float(t1u @ ru + t1p @ rp)
    return dict(x=(xu, xp), r=(ru, rp), d=(t1u.copy(), t1p.copy()), a=(au, ap), t1=(t1u, t1p),
                t2=(f - Ku, g - Kp)), rho


@functools.lru_cache(maxsize=None)
def bpcg1_restated(dim, n, kind):
    """bramble_pasciak_cg.py:125-141 once, in numpy; t1u as the device leaves it (:135 writes only the pressure half:
    the loop reads a_u where the reference reads t1u)."""
    s, C, f, g, dinv, k = system(dim, n, kind)
    A, B, minv = s.A, s.B, 1.0 / s.mass
    st, rho = bpcg1_start(dim, n, kind)
    (xu, xp), (ru, rp), (du, dp), (au, ap) = st["x"], st["r"], st["d"], st["a"]
    ku, kp = A @ du + B.T @ dp, B @ du + C @ dp                              # :125
    t2u, t2p = k * dinv * ku, kp                                             # :126
    t1u, t1p = -ku + A @ t2u, -kp + B @ t2u                                  # :127
    alpha = rho / float(du @ t1u + dp @ t1p)
    xu, xp = xu + alpha * du, xp + alpha * dp
    ru, rp = ru - alpha * t1u, rp - alpha * t1p
    au, ap = au - alpha * t2u, ap - alpha * t2p
    t1p = minv * (B @ au - ap)                                               # :135
    beta = float(au @ ru + t1p @ rp) / rho
    du, dp = beta * du + au, beta * dp + t1p
    cat = np.concatenate
    return dict(x=cat([xu, xp]), r=cat([ru, rp]), d=cat([du, dp]), a=cat([au, ap]), t1=cat([t1u, t1p]),
                t2=cat([t2u, t2p])), alpha, beta


def bpcg1_on_device(eng, dim, n, kind, with_c=True):
    """Phases 1 .. 5 of iteration 0 (nss_bpcg1_phases) from `bpcg1_start`; the operands are made here, under the
    overrides in force.  Returns ({name: [u; p]}, alpha, beta)."""
    import hipla
    from hipla import fused
    s, C, f, g, dinv, k = system(dim, n, kind)
    st, rho = bpcg1_start(dim, n, kind)
    A, B = hipla.SparseMatrix.from_scipy(s.A), hipla.SparseMatrix.from_scipy(s.B)
    Cm = hipla.SparseMatrix.from_scipy(C) if with_c else None
    vecs = {name: hipla.BlockVector([hipla.Vector.from_numpy(u), hipla.Vector.from_numpy(p)])
            for name, (u, p) in st.items()}
    loop = fused.Bpcg1Loop.try_create(A, B, Cm, hipla.DiagonalMatrix(dinv), hipla.DiagonalMatrix(1.0 / s.mass), k, vecs)
    assert loop is not None, fused.Bpcg1Loop.last_declined
    assert bool(loop.state.C) == with_c and bool(loop.state.C_work) == with_c
    loop.hist = eng.zeros(4)
    loop.state.hist = loop.hist.data_ptr()
    scal = np.zeros(16)
    scal[0], scal[5], scal[6] = rho, np.sqrt(abs(rho)), 0.0
    eng.upload(scal, loop.scal)
    loop.ctrl.zero_()
    eng._check(eng.lib.nss_bpcg1_phases(ctypes.byref(loop.state), 1, 5, 0, eng.stream))
    stop, _ = loop.poll()
    assert not stop
    scal = eng.to_host(loop.scal)
    assert eng.to_host(loop.hist)[0] == 1.0
    return {name: v.numpy() for name, v in vecs.items()}, float(scal[3]), float(scal[4])


BPCG1_SETTINGS = [dict(bpcg1_fold=fold, **direct) for fold in (-1, 0, 1) for direct in ({}, {"direct_rows": 0})]


@pytest.mark.parametrize("kind", C_KINDS)
@pytest.mark.parametrize("dim,n", SIZES)
def test_bpcg1_iteration_with_c_against_numpy(hip_engine, dim, n, kind):
    want, alpha, beta = bpcg1_restated(dim, n, kind)
    first = None
    for settings in BPCG1_SETTINGS:
        with hip_engine.overrides(**settings):
            got, a, b = bpcg1_on_device(hip_engine, dim, n, kind)
        err = worst(got, want)
        print("BPCG1 %d-D n=%d %s %s: %.3g of max-abs; alpha %.3g, beta %.3g off"
              % (dim, n, kind, settings, err, abs(a / alpha - 1.0), abs(b / beta - 1.0)))
        assert err <= BOUND, settings
        if first is None:
            first = got
        for name in want:
            np.testing.assert_array_equal(got[name], first[name], err_msg="%s %s" % (name, settings))
    # and C does enter: without it the pressure half of t2 (= kp, :126) is another vector
    if kind == "generator":
        without, _, _ = bpcg1_on_device(hip_engine, dim, n, kind, with_c=False)
        assert np.abs(without["t2"] - want["t2"]).max() > 1e-6 * np.abs(want["t2"]).max()


@functools.lru_cache(maxsize=None)
def minres_restated(dim, n, kind, steps=2):
    """minres.py:62-118 for `steps` iterations in numpy.  Returns the start (normalised v, z, gamma) and, of the last
    iteration, what it wrote: kz, v_new and z_new before :104-105 scale them (the loop stores them un-normalised),
    w_new, u; and the history."""
    s, C, f, g, dinv, _ = system(dim, n, kind)
    K = sp.bmat([[s.A, s.B.T], [s.B, C]], format="csr")
    P = np.concatenate([dinv, 1.0 / s.mass])
    v = np.concatenate([f, g])
    z = P * v
    gamma = float(np.sqrt(z @ v))
    z, v = z / gamma, v / gamma
    start = (v.copy(), z.copy(), gamma)
    u, v_old, w_old, w = np.zeros_like(v), np.zeros_like(v), np.zeros_like(v), np.zeros_like(v)
    eta_old, c_old, c, s_old, sn, res_old, hist = gamma, 1.0, 1.0, 0.0, 0.0, gamma, [1.0]
    for _ in range(steps):
        kz = K @ z                                                           # :97
        delta = float(kz @ z)
        v_raw = kz - delta * v - gamma * v_old                               # :99
        z_raw = P * v_raw                                                    # :101
        gamma_new = float(np.sqrt(z_raw @ v_raw))
        a0 = c * delta - c_old * sn * gamma                                  # :107-113
        a1 = np.sqrt(a0 * a0 + gamma_new * gamma_new)
        a2 = sn * delta + c_old * c * gamma
        a3 = s_old * gamma
        c_new, s_new = a0 / a1, gamma_new / a1
        w_new = (z - a3 * w_old - a2 * w) / a1                               # :115-116
        u = u + c_new * eta_old * w_new                                      # :118
        res = abs(s_new) * res_old
        hist.append(res / start[2])
        out = dict(kz=kz, v=v_raw, z=z_raw, w=w_new, u=u)
        v_old, v, z = v, v_raw / gamma_new, z_raw / gamma_new
        w_old, w = w, w_new
        eta_old, s_old, sn, c_old, c, gamma, res_old = -s_new * eta_old, sn, s_new, c, c_new, gamma_new, res
    return start, out, np.array(hist)


def minres_on_device(eng, dim, n, kind, steps=2):
    """`steps` iterations of the fused loop from the start state of minres.py:62-75; what the last one wrote."""
    import hipla
    from hipla import fused
    s, C, f, g, dinv, _ = system(dim, n, kind)
    (v0, z0, gamma), _, _ = minres_restated(dim, n, kind, steps)
    A, B = hipla.SparseMatrix.from_scipy(s.A), hipla.SparseMatrix.from_scipy(s.B)
    K = hipla.BlockMatrix([[A, B.T], [B, hipla.SparseMatrix.from_scipy(C)]])
    P = hipla.BlockMatrix([[hipla.DiagonalMatrix(dinv), None], [None, hipla.DiagonalMatrix(1.0 / s.mass)]])

    def block(values=None):
        values = np.zeros(s.ndof) if values is None else values
        return hipla.BlockVector([hipla.Vector.from_numpy(values[:s.n_u]), hipla.Vector.from_numpy(values[s.n_u:])])

    u, kz = block(), block()
    v_ring, w_ring, z_ring = [block(), block(v0), block()], [block(), block(), block()], [block(), block(z0)]
    loop = fused.MinresLoop.try_create(K, P, u, v_ring, w_ring, z_ring, kz)
    assert loop is not None, fused.MinresLoop.last_declined
    assert loop.state.C and loop.state.C_work
    errors, hit = loop.run(gamma, 0.0, steps)
    assert not hit and len(errors) == steps + 1
    k = steps                                              # ring slots of the last iteration's new vectors
    return dict(kz=kz.numpy(), v=v_ring[(k + 1) % 3].numpy(), z=z_ring[(k + 1) % 2].numpy(),
                w=w_ring[(k + 1) % 3].numpy(), u=u.numpy()), np.array(errors)


MINRES_SETTINGS = ([dict(minres_fold=fold, **direct) for fold in (-1, 0, 1) for direct in ({}, {"direct_rows": 0})]
                   + [dict(minres_fuse=0), dict(minres_fuse=2)])


@pytest.mark.parametrize("kind", C_KINDS)
@pytest.mark.parametrize("dim,n", SIZES)
def test_minres_iterations_with_c_against_numpy(hip_engine, dim, n, kind):
    _, want, hist = minres_restated(dim, n, kind)
    first = None
    for settings in MINRES_SETTINGS:
        with hip_engine.overrides(**settings):
            got, errors = minres_on_device(hip_engine, dim, n, kind)
        err = worst(got, want)
        print("MINRES %d-D n=%d %s %s: %.3g of max-abs, history %.3g off"
              % (dim, n, kind, settings, err, np.abs(errors / hist - 1.0).max()))
        assert err <= BOUND, settings
        np.testing.assert_allclose(errors, hist, rtol=1e-12)
        if first is None:
            first = got, errors
        for name in want:
            np.testing.assert_array_equal(got[name], first[0][name], err_msg="%s %s" % (name, settings))
        np.testing.assert_array_equal(errors, first[1])


# ---- a stored zero C is C = None -------------------------------------------------------------------------------------
GRID12 = sc.params(2, 12, 1.0, "jacobi")


@pytest.mark.parametrize("stored", ["nnz=0", "explicit zeros"])
@pytest.mark.parametrize("solver", sc.SOLVERS)
def test_a_stored_zero_c_gives_the_bits_of_no_c(hip_engine, solver, stored):
    case = sc.StabCase(GRID12)
    n_p = case.system.n_p
    zero = sp.csr_matrix((n_p, n_p))
    if stored == "explicit zeros":
        zero = sp.csr_matrix((np.zeros(case.C.nnz), case.C.indices.copy(), case.C.indptr.copy()), shape=case.C.shape)
        assert zero.nnz == case.C.nnz > 0
    runs = []
    for C in (None, zero):
        with fused_loops_counted() as counts:
            x, errors, _, _ = sc.solve(solver, case, sc.device_operands(case, C), tol=0.0, maxsteps=40)
        assert counts[solver] == 1
        runs.append((x, errors))
    assert len(runs[0][1]) >= 40
    np.testing.assert_array_equal(runs[1][1], runs[0][1])
    np.testing.assert_array_equal(runs[1][0], runs[0][0])


# ---- warm start ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("solver", sc.SOLVERS)
def test_warm_start_is_updated_in_place(hip_engine, solver):
    """A `solution` / `sol` on 2-D n = 12: the vector handed in comes back, and its residual WITH C is that of the
    protocol path from the same start (within the factor 10 of check_solution)."""
    case = sc.StabCase(GRID12)
    rng = np.random.default_rng(7)
    warm = (0.1 * rng.standard_normal(case.system.n_u), 0.1 * rng.standard_normal(case.system.n_p))
    K, b = case.matrix(), case.rhs
    with protocol_path():
        xp, ep, _, same = sc.solve(solver, case, sc.device_operands(case), warm=warm)
    assert same and ep[-1] < sc.TOL
    with fused_loops_counted() as counts:
        x, errors, _, same = sc.solve(solver, case, sc.device_operands(case), warm=warm)
    assert counts[solver] == 1 and same and errors[-1] < sc.TOL
    res, res_p = np.linalg.norm(b - K @ x), np.linalg.norm(b - K @ xp)
    print("WARM %s: residual %.3g (protocol %.3g), %d iterations (protocol %d)"
          % (solver, res, res_p, len(errors) - 1, len(ep) - 1))
    assert res <= 10 * max(res_p, 1e-12 * np.linalg.norm(b))
    assert np.linalg.norm(b - K @ np.concatenate(warm)) > 1e3 * res          # (it did start somewhere else)


# ---- stop handling ---------------------------------------------------------------------------------------------------
def same_iterate(x, want):
    """Iterates of the two paths after the same few iterations: 1e-11 of max-abs (tests/test_saddle_loop_edges_gpu.py:
    a reordering moves an iterate by ~1e-15, a write after the stop by a whole step)."""
    return np.abs(x - want).max() <= 1e-11 * np.abs(want).max()


@pytest.mark.parametrize("solver", sc.SOLVERS)
def test_max_steps_below_the_iteration_count(hip_engine, solver):
    case = sc.StabCase(GRID12)
    with protocol_path():
        xp, ep, text_p, _ = sc.solve(solver, case, sc.device_operands(case), maxsteps=5)
    with fused_loops_counted() as counts:
        x, errors, text, _ = sc.solve(solver, case, sc.device_operands(case), maxsteps=5)
    assert counts[solver] == 1 and len(errors) == len(ep) == (5 if solver == "bpcg1" else 6)
    assert "Warning" in text and "Warning" in text_p
    np.testing.assert_allclose(errors, ep, rtol=1e-8)
    assert same_iterate(x, xp)


@pytest.mark.parametrize("solver", sc.SOLVERS)
def test_tolerance_reached_at_iteration_one(hip_engine, solver):
    """2-D n = 3 with a tolerance between the first two history entries: the loop stops at iteration 1 although a
    whole chunk of iterations is enqueued behind it, and x is the protocol path's."""
    case = sc.StabCase(sc.params(2, 3, 0.5, "jacobi"))
    with protocol_path():
        _, probe, _, _ = sc.solve(solver, case, sc.device_operands(case), tol=0.0, maxsteps=3)
    assert probe[0] == 1.0 and probe[1] < 1.0
    tol = 0.5 * (1.0 + probe[1])
    with protocol_path():
        xp, ep, _, _ = sc.solve(solver, case, sc.device_operands(case), tol=tol, maxsteps=50)
    with fused_loops_counted() as counts:
        x, errors, _, _ = sc.solve(solver, case, sc.device_operands(case), tol=tol, maxsteps=50)
    assert counts[solver] == 1 and len(errors) == len(ep) == 2
    np.testing.assert_allclose(errors, ep, rtol=1e-12)
    assert np.abs(xp).max() > 0.0 and same_iterate(x, xp)
