"""Fast diagonalisation on the product engine: the contraction kernel of csrc/fdm.hip on its own against
`numpy.einsum` in long double, the solve ``nss_fdm_solve_f64`` through `hipla.FastDiagonalization` against the pressure
operator on the host, and `NavierStokes.SetProjection("fdm")` through the device-resident stepper against a "cg" twin.

Bounds.  The contraction, per output: the kernel sums its n products over j ascending with one fma each, so it errs by
at most gamma_n (|M| |X|) of that output; the bound is 2 (n + 2) 2^-53 (|M| |X|), the dot-product bound with a factor 2,
derived and not measured.  The scaled epilogue adds the rounding of 1 / s and of the product: |mult| (2 n + 7) 2^-53
(|M| |X|).  The solve: residual <= max(10 x that of the numpy restatement, 1e-14) |rhs|.  The stepper: 1e-9 |u| against a
twin whose CG projection runs to 1e-13, both with the velocity solve at 1e-12; |B u| <= 1e-12 x the largest |B raw| of
the run, read from the twin."""

import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

from oracle import krylov_ref as kr

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
LD = np.longdouble
SENT = -7.25                       # what output buffers hold before a launch
GUARD = 96                         # doubles in front of and behind an output


# ---- 1. the contraction alone -----------------------------------------------------------------------------------------
# one tile; one past a tile in each of the three extents; both instantiations (inner == 1: lines); 1 < inner < 64;
# more than one tile of i for the lines, more K-steps than one, and more workgroups than a grid's y / z extent takes
SHAPES = [(1, 1, 1), (3, 1, 7), (7, 2, 1), (5, 17, 1), (65, 33, 1), (1, 5, 3), (2, 16, 16), (3, 17, 5), (1, 67, 64),
          (2, 33, 130), (1, 136, 70), (66, 67, 1), (70000, 2, 2)]


def operands(shape, seed=0):
    outer, n, inner = shape
    rng = np.random.default_rng(seed + 1000 * n + inner)
    M = rng.standard_normal((n, n))
    if n > 1:
        assert abs(M - M.T).max() > 0.1            # asymmetric: a symmetric M hides a swapped index
    return M, rng.standard_normal((outer, n, inner))


def guarded_output(eng, count):
    """(the whole sentinel-filled buffer, its view of `count` doubles behind the front guard)."""
    whole = eng.from_host(np.full(count + 2 * GUARD, SENT))
    return whole, eng.view(whole, GUARD, GUARD + count)


def reference(M, X, transpose):
    """(M X in long double, |M| |X|) along the middle axis."""
    Mo = M.T if transpose else M
    want = np.einsum("ij,ojc->oic", Mo.astype(LD), X.astype(LD))
    return want, np.einsum("ij,ojc->oic", np.abs(Mo), np.abs(X))


def contract(eng, M, X, transpose, y):
    outer, n, inner = X.shape
    d_m, d_x = eng.from_host(M.ravel()), eng.from_host(X.ravel())
    rc = eng.lib.nss_fdm_contract_f64(outer, n, inner, d_m.data_ptr(), transpose, d_x.data_ptr(), y.data_ptr(), eng.stream)
    assert rc == 0, eng.lib.nss_last_error()
    eng.synchronize()
    assert np.array_equal(eng.to_host(d_x), X.ravel()) and np.array_equal(eng.to_host(d_m), M.ravel())


def check_guards(eng, whole, count):
    host = eng.to_host(whole)
    assert (host[:GUARD] == SENT).all() and (host[GUARD + count:] == SENT).all()


@pytest.mark.parametrize("transpose", [0, 1])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_contraction_against_einsum(hip_engine, shape, transpose):
    eng = hip_engine
    M, X = operands(shape)
    whole, y = guarded_output(eng, X.size)
    contract(eng, M, X, transpose, y)
    got = eng.to_host(y).reshape(shape)
    want, scale = reference(M, X, transpose)
    err = np.abs(np.asarray(got.astype(LD) - want, dtype=np.float64))
    bound = 2 * (shape[1] + 2) * U * scale
    print("contraction %s transpose=%d: max err / bound = %.3f" % (shape, transpose, float((err / bound).max())))
    assert (err <= bound).all(), (np.argwhere(err > bound)[:8], float((err / bound).max()))
    check_guards(eng, whole, X.size)


@pytest.mark.parametrize("transpose", [0, 1])
@pytest.mark.parametrize("shape,extents,axis", [((2, 17, 5), (2, 17, 5), 1), ((1, 5, 3), (5, 3), 0), ((5, 3, 1), (5, 3), 1),
                                                ((1, 4, 6), (4, 2, 3), 0)])
def test_scaled_epilogue_against_the_host_formula(hip_engine, shape, extents, axis, transpose):
    """Y of cell p times 1 / ((lambda_0[p_0] + lambda_1[p_1]) + lambda_2[p_2]) of the cell's multi-index in `extents`
    (two or three axes; the contraction runs along `axis`), with one sum made exactly 0: its cell gives exactly 0."""
    eng = hip_engine
    M, X = operands(shape, seed=3)
    rng = np.random.default_rng(17)
    lam = [1.0 + rng.random(e) for e in extents]
    null = tuple(e - 1 for e in extents)                    # the last cell: (l_0 + l_1) + l_2 == 0 exactly
    head = lam[0][null[0]] + lam[1][null[1]]
    if len(extents) == 3:
        lam[2][null[2]] = -head
    else:
        lam[1][null[1]] = -lam[0][null[0]]
    sums = lam[0].reshape((-1,) + (1,) * (len(extents) - 1))
    for a in range(1, len(extents)):
        sums = sums + lam[a].reshape((1,) * a + (-1,) + (1,) * (len(extents) - 1 - a))
    threshold = 1e-12 * abs(sums).max()
    assert sums[null] == 0.0 and int((abs(sums) <= threshold).sum()) == 1
    mult = np.where(abs(sums) <= threshold, 0.0, 1.0 / np.where(sums == 0.0, 1.0, sums)).reshape(shape)
    whole, y = guarded_output(eng, X.size)
    d_m, d_x, d_lam = eng.from_host(M.ravel()), eng.from_host(X.ravel()), eng.from_host(np.concatenate(lam))
    ext = (C.c_int64 * len(extents))(*extents)
    rc = eng.lib.nss_fdm_contract_scaled_f64(shape[0], shape[1], shape[2], d_m.data_ptr(), transpose, d_x.data_ptr(),
                                             y.data_ptr(), len(extents), ext, d_lam.data_ptr(), threshold, eng.stream)
    assert rc == 0, eng.lib.nss_last_error()
    got = eng.to_host(y).reshape(shape)
    want, scale = reference(M, X, transpose)
    err = np.abs(np.asarray(got.astype(LD) - want * mult.astype(LD), dtype=np.float64))
    bound = (2 * shape[1] + 7) * U * scale * np.abs(mult)
    assert (err <= bound).all(), (np.argwhere(err > bound)[:8], float((err / np.maximum(bound, 1e-300)).max()))
    assert got.reshape(extents)[null] == 0.0 and int((got == 0.0).sum()) == 1
    check_guards(eng, whole, X.size)


def test_contraction_refusals(hip_engine):
    """NULL pointers, an extent below 1, more than 2^31 - 1 cells, y == x, a dim that is not 2 or 3, extents of another
    size: non-zero with a message, and nothing is launched (the output keeps its sentinel)."""
    eng, lib = hip_engine, hip_engine.lib
    M, X = operands((2, 3, 4))
    d_m, d_x = eng.from_host(M.ravel()), eng.from_host(X.ravel())
    whole, y = guarded_output(eng, X.size)
    m, x, out, st = d_m.data_ptr(), d_x.data_ptr(), y.data_ptr(), eng.stream
    calls = [(2, 3, 4, None, 0, x, out), (2, 3, 4, m, 0, None, out), (2, 3, 4, m, 0, x, None), (2, 3, 4, m, 0, x, x),
             (0, 3, 4, m, 0, x, out), (2, 0, 4, m, 0, x, out), (2, 3, -1, m, 0, x, out),
             (2 ** 16, 3, 2 ** 15, m, 0, x, out), (2 ** 40, 2 ** 40, 2 ** 40, m, 0, x, out)]
    for args in calls:
        assert lib.nss_fdm_contract_f64(*args, st) != 0, args
        assert b"fdm_contract" in lib.nss_last_error()
    lam = eng.from_host(np.ones(9))
    ext3, ext2 = (C.c_int64 * 3)(2, 3, 4), (C.c_int64 * 3)(2, 3, 5)
    for dim, ext, lam_ptr in ((1, ext3, lam.data_ptr()), (4, ext3, lam.data_ptr()), (3, None, lam.data_ptr()),
                              (3, ext3, None), (3, ext2, lam.data_ptr())):
        assert lib.nss_fdm_contract_scaled_f64(2, 3, 4, m, 0, x, out, dim, ext, lam_ptr, 0.0, st) != 0, dim
        assert b"fdm_contract_scaled" in lib.nss_last_error()
    eng.synchronize()
    assert (eng.to_host(whole) == SENT).all()


# ---- 2. the solve -----------------------------------------------------------------------------------------------------
SOLVES = {"2d_n2": (2, 2, 1), "2d_n5": (2, 5, 1), "2d_n12": (2, 12, 1), "2d_n33": (2, 33, 1), "3d_n2": (3, 2, 1),
          "3d_n4": (3, 4, 1), "3d_n7": (3, 7, 1), "3d_n17": (3, 17, 1), "3d_n5_inflated3": (3, 5, 3)}


def pressure_operator(case):
    from staggered_grid import mac_stokes
    dim, n, bs = SOLVES[case]
    s = mac_stokes(dim, n, 0.01)
    s = s.inflate(bs) if bs > 1 else s
    Lp = (s.B @ sp.diags(np.full(s.n_u, 1.0 / s.h ** s.dim)) @ s.B.T).tocsr()
    Lp.sort_indices()
    return s, Lp


@pytest.mark.parametrize("case", sorted(SOLVES))
def test_solve_against_the_operator(hip_engine, case):
    import hipla
    eng = hip_engine
    s, Lp = pressure_operator(case)
    inv = hipla.FastDiagonalization(Lp, (s.n,) * s.dim)
    assert inv.handle is not None and inv.iterations == 0 and inv.factors.zeroed == 1
    rhs = s.B @ np.random.default_rng(3).standard_normal(s.n_u)
    size = np.linalg.norm(rhs)
    host = np.linalg.norm(Lp @ inv.factors.solve(rhs) - rhs) / size
    d_rhs = eng.from_host(rhs)
    whole, phi = guarded_output(eng, s.n_p)
    assert inv.solve_resident(d_rhs, phi) == 0
    first = eng.to_host(phi).copy()
    res = np.linalg.norm(Lp @ first - rhs) / size
    print("%s: residual %.3g (numpy restatement %.3g), |mean phi| / max |phi| %.3g"
          % (case, res, host, abs(first.mean()) / abs(first).max()))
    assert res <= max(10 * host, 1e-14)
    assert abs(first.mean()) <= 1e-13 * abs(first).max()
    assert np.array_equal(eng.to_host(d_rhs), rhs)                        # rhs is unchanged bit for bit
    check_guards(eng, whole, s.n_p)
    eng.upload(np.full(s.n_p, SENT), phi)
    inv.solve_resident(d_rhs, phi)
    assert np.array_equal(eng.to_host(phi), first)                        # a second solve reproduces the first
    x, y = hipla.Vector.from_numpy(rhs), hipla.Vector(s.n_p)              # ... and so does the protocol's statement
    y.data = inv * x
    assert np.array_equal(y.numpy(), first) and np.array_equal(x.numpy(), rhs)
    x.data = inv * x                                                       # (x over itself: through a copy)
    assert np.array_equal(x.numpy(), first)


def test_solve_refusals(hip_engine):
    """The refusals of create and solve: non-zero with a message, no handle, nothing launched."""
    import hipla
    eng, lib = hip_engine, hip_engine.lib
    q = np.eye(3)
    lam = np.ones(3)
    qs, lams = (C.c_void_p * 3)(*[q.ctypes.data] * 3), (C.c_void_p * 3)(*[lam.ctypes.data] * 3)
    none = (C.c_void_p * 3)(None, None, None)
    out = C.c_void_p()

    def ext(*e):
        return (C.c_int64 * 3)(*e)
    for args in [(3, None, qs, lams, 0.0, C.byref(out)), (3, ext(3, 3, 3), None, lams, 0.0, C.byref(out)),
                 (3, ext(3, 3, 3), qs, None, 0.0, C.byref(out)), (3, ext(3, 3, 3), qs, lams, 0.0, None),
                 (3, ext(3, 3, 3), none, lams, 0.0, C.byref(out)), (3, ext(3, 3, 3), qs, none, 0.0, C.byref(out)),
                 (1, ext(3, 3, 3), qs, lams, 0.0, C.byref(out)), (4, ext(3, 3, 3), qs, lams, 0.0, C.byref(out)),
                 (3, ext(3, 0, 3), qs, lams, 0.0, C.byref(out)), (2, ext(3, -2, 3), qs, lams, 0.0, C.byref(out)),
                 (2, ext(2 ** 16, 2 ** 15, 1), qs, lams, 0.0, C.byref(out)),
                 (3, ext(2 ** 31, 2 ** 31, 2 ** 31), qs, lams, 0.0, C.byref(out))]:
        assert lib.nss_fdm_create(*args) != 0, args[:2]
        assert b"fdm_create" in lib.nss_last_error() and not out.value
    s, Lp = pressure_operator("2d_n5")
    inv = hipla.FastDiagonalization(Lp, (5, 5))
    d_rhs = eng.from_host(np.ones(25))
    whole, phi = guarded_output(eng, 25)
    for args in [(None, d_rhs.data_ptr(), phi.data_ptr()), (inv.handle.ptr, None, phi.data_ptr()),
                 (inv.handle.ptr, d_rhs.data_ptr(), None), (inv.handle.ptr, phi.data_ptr(), phi.data_ptr())]:
        assert lib.nss_fdm_solve_f64(*args, eng.stream) != 0
        assert b"fdm_solve" in lib.nss_last_error()
    eng.synchronize()
    assert (eng.to_host(whole) == SENT).all()
    assert lib.nss_fdm_destroy(None) == 0


# ---- 3. the stepper -----------------------------------------------------------------------------------------------------
TAU = 0.05
WALLS = {"x-": 1.0, "x+": 0.0}
GRIDS = {"2d": (2, 8, (0.0, 2.0)), "3d": (3, 5, (0.0, 2.0, -1.0))}
SIZES = [0.05, 0.03, 0.045, 0.02]
TIGHT = dict(precision=(1e-12, 1e-13))
MODES = {"fixed": lambda k: {}, "timesteps": lambda k: dict(timesteps=SIZES[k]), "pseudo": lambda k: dict(pseudo=True)}


def fresh(grid, scheme="euler", buoyant=False, projection=None):
    """A `NavierStokes` with a seeded divergence-free start (max |u| tau / h about 0.1), a seeded force and start
    pressure, optionally a buoyant scalar; `projection`: what `SetProjection` is called with (None: it is not called)."""
    import hipla
    from templates.NavierStokesSIMPLE_iterative import NavierStokes, SyntheticMesh
    dim, n, beta = GRIDS[grid]
    ns = NavierStokes(SyntheticMesh(1.0 / n, dim=dim), nu=0.01, inflow="inlet", outflow="outlet", wall="wall|cyl",
                      uin=None, timestep=TAU, order=0, time_scheme=scheme)
    s = ns.system
    assert s.block_size == 1 and s.n == n
    ns.f.vec.data = hipla.Vector.from_numpy(0.5 * s.h ** s.dim * np.random.default_rng(8).standard_normal(s.n_u))
    u0 = 0.2 * kr.project(s.B, np.full(s.n_u, s.h ** s.dim), np.random.default_rng(2).standard_normal(s.n_u))[0]
    ns.gfu.data = hipla.Vector.from_numpy(u0)
    p0 = np.random.default_rng(4).standard_normal(s.n_p)
    ns.gfup.data = hipla.Vector.from_numpy(0.01 * (p0 - p0.mean()))
    if buoyant:
        ns.AddScalar(initial=np.random.default_rng(6).random(s.n_p), precision=1e-14, maxsteps=5000, kappa=0.8,
                     dirichlet=WALLS, buoyancy=beta, t_ref=0.5)
    if projection is not None:
        ns.SetProjection(projection)
    return ns


def rel(a, b):
    return np.linalg.norm(np.asarray(a) - b) / np.linalg.norm(b)


def only_stepper(ns):
    assert ns.advance_declined is None and len(ns._steppers) == 1, (ns.advance_declined, list(ns._steppers))
    return next(iter(ns._steppers.values()))


def state(ns):
    out = [ns.gfu.numpy().copy(), ns.gfup.numpy().copy()]
    return out + ([ns.temperature.numpy().copy()] if ns._scalar is not None else [])


STEPPER_CASES = [(grid, scheme, buoyant, mode) for grid in sorted(GRIDS) for scheme in ("euler", "cnab2")
                 for buoyant in (False, True) for mode in sorted(MODES) if not (mode == "pseudo" and buoyant)]


@pytest.mark.parametrize("grid,scheme,buoyant,mode", STEPPER_CASES)
def test_advance_against_the_cg_twin(hip_engine, grid, scheme, buoyant, mode):
    """`Advance(4)` after `SetProjection("fdm")` against `Advance(4, precision=(1e-12, 1e-13))` on a "cg" twin.  The
    scale of the divergence bound, the largest |B raw| of the run, comes from a second "cg" object that takes the steps
    one call at a time (the bits of one call of four), so that its stepper's `raw` can be read after every step; of the
    pseudo time stepping it takes the first step only: a relaxation, whose raw = mstar^-1 (-A u) decays from step to
    step, and whose second projection per step runs on rounding noise -- thousands of CG iterations per call.

    Measured: |u_fdm - u_cg| / |u| is 2e-16 to 3e-14 for the fixed and prescribed steps (31 or 32 CG iterations per
    projection on the twin); for the pseudo time stepping 2e-13 (2-D) and 3.1e-10 (3-D), where the twin's CG runs into
    its cap of 5000 iterations on a B u that is rounding noise with a component along the constants -- that figure is
    the twin's error, not the direct solve's.  div_norm is 1e-17 to 2e-16 against |B raw| of 0.02 to 1.1."""
    eng = hip_engine
    direct, twin, ruler = fresh(grid, scheme, buoyant, "fdm"), fresh(grid, scheme, buoyant), fresh(grid, scheme, buoyant)
    kw = MODES[mode]
    rec = direct.Advance(4, **kw(slice(0, 4)), **TIGHT)
    ref = twin.Advance(4, **kw(slice(0, 4)), **TIGHT)
    assert ref.projection == "cg"
    its = ref.proj_iterations.tolist()
    B, scale = ruler.system.B, 0.0
    for k in range(1 if mode == "pseudo" else 4):
        ruler.Advance(1, **kw(slice(k, k + 1)), **TIGHT)
        scale = max(scale, float(np.linalg.norm(B @ eng.to_host(only_stepper(ruler).raw))))
    stepper = only_stepper(direct)
    assert stepper.cg_p is None and stepper.pre_p is None and stepper.fdm is direct._fdm
    assert direct._stepper_shared["fdm"] is direct._fdm and stepper.projection == "fdm"
    assert rec.projection == "fdm" and rec.proj_iterations.shape == (4,) and (rec.proj_iterations == 0).all()
    assert min(its) > 0
    err = rel(direct.gfu.numpy(), twin.gfu.numpy())
    print("%s %s buoyant=%s %s: |u_fdm - u_cg| / |u| %.3g, div_norm %s, largest |B raw| %.3g, CG iterations %s"
          % (grid, scheme, buoyant, mode, err, rec.div_norm, scale, its))
    assert err <= 1e-9
    if buoyant:
        assert rel(direct.temperature.numpy(), twin.temperature.numpy()) <= 1e-9
    assert (rec.div_norm <= 1e-12 * scale).all()
    assert rec.time_scheme == ("euler" if mode == "pseudo" else scheme)


@pytest.mark.parametrize("scheme", ["euler", "cnab2"])
@pytest.mark.parametrize("mode", ["fixed", "timesteps"])
def test_split_advance_is_bit_identical(hip_engine, scheme, mode):
    """`Advance(2); Advance(2)` has the bits of `Advance(4)`: velocity, potential, temperature, the record."""
    one, two = fresh("2d", scheme, True, "fdm"), fresh("2d", scheme, True, "fdm")
    kw = MODES[mode]
    rec = one.Advance(4, **kw(slice(0, 4)))
    first, second = two.Advance(2, **kw(slice(0, 2))), two.Advance(2, **kw(slice(2, 4)))
    for a, b in zip(state(one), state(two)):
        assert np.array_equal(a, b)
    assert np.array_equal(rec.div_norm, np.concatenate([first.div_norm, second.div_norm]))
    assert np.array_equal(rec.kinetic_energy, np.concatenate([first.kinetic_energy, second.kinetic_energy]))
    assert np.array_equal(rec.mstar_iterations, np.concatenate([first.mstar_iterations, second.mstar_iterations]))


@pytest.mark.parametrize("grid", sorted(GRIDS))
def test_amg_velocity_solve_with_the_direct_projection(hip_engine, grid):
    """`inner_pre="amg"` with "fdm": the hierarchy of Lp is not built, the steppers of one object share the handle, and
    the velocity agrees with the Jacobi stepper's at `TIGHT`."""
    amg, jac = fresh(grid, "euler", True, "fdm"), fresh(grid, "euler", True, "fdm")
    rec = amg.Advance(3, inner_pre="amg", **TIGHT)
    jac.Advance(3, **TIGHT)
    stepper = only_stepper(amg)
    assert stepper.pre_m is not None and stepper.pre_p is None and stepper.cg_p is None
    assert rec.projection == "fdm" and (rec.proj_iterations == 0).all()
    assert rel(amg.gfu.numpy(), jac.gfu.numpy()) <= 1e-9
    amg.Advance(1, **TIGHT)                                  # a second stepper of the same object: the same handle
    assert len(amg._steppers) == 2 and len({id(st.fdm) for st in amg._steppers.values()}) == 1
    with pytest.raises(ValueError):
        amg.Advance(2, timesteps=[0.01, 0.02], inner_pre="amg")


def test_the_switch_moves_between_calls(hip_engine):
    """One object: "fdm" steps, back to "cg", "fdm" again -- every call takes the stepper of its projection, the direct
    one is built once, and the velocity follows an all-"cg" twin at `TIGHT`."""
    mixed, twin = fresh("2d", "cnab2", True, "fdm"), fresh("2d", "cnab2", True)
    recs = [mixed.Advance(2, **TIGHT)]
    handle = mixed._fdm
    mixed.SetProjection("cg")
    recs.append(mixed.Advance(1, **TIGHT))
    mixed.SetProjection("fdm")
    recs.append(mixed.Advance(1, **TIGHT))
    twin.Advance(4, **TIGHT)
    assert [r.projection for r in recs] == ["fdm", "cg", "fdm"] and mixed._fdm is handle and len(mixed._steppers) == 2
    assert (recs[1].proj_iterations > 0).all() and (recs[2].proj_iterations == 0).all()
    assert rel(mixed.gfu.numpy(), twin.gfu.numpy()) <= 1e-9
    assert rel(mixed.temperature.numpy(), twin.temperature.numpy()) <= 1e-9


@pytest.mark.parametrize("scheme", ["euler", "cnab2"])
def test_an_object_left_at_cg_keeps_its_bits(hip_engine, scheme):
    """No shared state: an object left at "cg" after another object has switched and stepped has the bits -- state,
    record, iteration counts -- of one that ran before `SetProjection` was ever called."""
    before = fresh("2d", scheme, True)
    rec_before = before.Advance(3)
    other = fresh("2d", scheme, True, "fdm")
    other.Advance(3)
    after = fresh("2d", scheme, True)
    rec_after = after.Advance(3)
    assert after._fdm is None and "fdm" not in after._stepper_shared and only_stepper(after).fdm is None
    for a, b in zip(state(before), state(after)):
        assert np.array_equal(a, b)
    for name in ("mstar_iterations", "proj_iterations", "scalar_iterations", "div_norm", "kinetic_energy", "wall_flux"):
        assert np.array_equal(getattr(rec_before, name), getattr(rec_after, name)), name
    assert rec_after.projection == "cg"


def test_statements_on_the_device_follow_the_switch(hip_engine):
    """`DoTimeStep` and `Project` with "fdm" on the product engine: `invproj` launches the direct solve."""
    import contextlib
    import io
    import hipla
    direct, twin = fresh("3d", "euler", False, "fdm"), fresh("3d", "euler", False)
    for ns in (direct, twin):
        ops = ns._time_stepping_operators()
        ops["invmstar"].precision, ops["invmstar"].maxsteps = 1e-12, 5000
    ops = twin._time_stepping_operators()
    ops["invproj"].precision, ops["invproj"].maxsteps = 1e-13, 20000
    inv = direct._time_stepping_operators()["invproj"]
    assert isinstance(inv, hipla.FastDiagonalization) and inv.handle is not None
    with contextlib.redirect_stdout(io.StringIO()):
        for _ in range(2):
            direct.DoTimeStep()
            twin.DoTimeStep()
    assert rel(direct.gfu.numpy(), twin.gfu.numpy()) <= 1e-9 and inv.iterations == 0
