"""Fast diagonalisation on the components of an interleaved vector, on the product engine: the batched, pitched kernel
of csrc/fdm_components.hip on synthetic handles against the formula in long double, one pass on its own against
`numpy.einsum`, the refusals of the entry points, and `hipla.ComponentFastDiagonalization` on the operators of the grid.

Bounds, derived and not measured, with u = 2^-53.  One pass along an axis of extent n sums n products over j ascending
with one fma each: it errs by at most gamma_n (|Q| |x|) per output; as in tests/test_fdm_gpu.py the bound is
2 (n + 2) u (|Q| |x|), the factor 2 covering the products of the (1 + gamma) of a chain.  The shifted epilogue adds, on
positive lambda and sigma >= 0: two additions in the sum of the eigenvalues (2 u), the product with sigma (u), the
addition of the mass (u), the reciprocal (u) and the product (u): (2 n + 10) u |mult| (|Q| |x|) for a scaled pass.  A
solve is 2 dim passes, each erring relative to what it is handed, so per entry

    |out - exact| <= c u (|Q_0| (x) .. ) |mult| (|Q_0^T| (x) .. ) |rhs|,      c = sum over the 2 dim passes of 2 (n_a + 2), + 6.

The real operators: residual <= max(10 x that of the numpy restatement, 1e-14) |rhs|."""

import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
LD = np.longdouble
SENT = -7.25                       # what output buffers hold before a launch
GUARD = 96                         # doubles in front of and behind an output


# ---- layouts ----------------------------------------------------------------------------------------------------------
def mac_layout(dim, n):
    from staggered_grid import mac_stokes
    s = mac_stokes(dim, n, 0.01)
    comps = s.component_ids
    pitch = 2 * n - 1 if dim == 2 else 3 * n * n - 2 * n
    return dict(n_total=s.n_u, pitch=pitch, bases=[int(g.flat[0]) for g in comps], extents=[g.shape for g in comps])


def single(extents, base=0, pitch=None, tail=0):
    slab = int(np.prod(extents[1:]))
    pitch = slab if pitch is None else pitch
    return dict(n_total=base + (extents[0] - 1) * pitch + slab + tail, pitch=pitch, bases=[base], extents=[tuple(extents)])


LAYOUTS = {
    "contiguous_2x17x5": single((2, 17, 5)),
    "gaps_3x4x5": single((3, 4, 5), base=3, pitch=29, tail=4),
    "mac3d_n2": mac_layout(3, 2),
    "mac3d_n5": mac_layout(3, 5),
    "mac2d_n5": mac_layout(2, 5),
    "two_large": dict(n_total=3 * 330, pitch=330, bases=[1, 199], extents=[(2, 66, 3), (3, 2, 65)]),
    "tile_65x3x2": single((65, 3, 2), base=1, pitch=7, tail=2),
    "tile_2x66x3": single((2, 66, 3), base=1, pitch=199, tail=2),
    "tile_3x2x65": single((3, 2, 65), base=1, pitch=131, tail=2),
    "tile_65x4": single((65, 4), base=1, pitch=5, tail=2),
    "tile_4x65": single((4, 65), base=1, pitch=66, tail=2),
    "one_1x4x3": single((1, 4, 3), base=2, pitch=12, tail=1),
    "one_4x1x3": single((4, 1, 3), base=2, pitch=4, tail=1),
    "one_4x3x1": single((4, 3, 1), base=2, pitch=4, tail=1),
    "one_1x5": single((1, 5), base=2, pitch=5, tail=1),
    "one_5x1": single((5, 1), base=2, pitch=2, tail=1),
}


def ids_of(layout):
    """The flat ids of every component, shaped by its extents: base + k * pitch + (j * e_2 + i)."""
    out = []
    for base, ext in zip(layout["bases"], layout["extents"]):
        k = np.arange(ext[0]).reshape((-1,) + (1,) * (len(ext) - 1))
        out.append(base + k * layout["pitch"] + np.arange(int(np.prod(ext[1:]))).reshape(ext[1:]))
    flat = np.concatenate([g.ravel() for g in out])
    assert len(set(flat.tolist())) == flat.size and flat.min() >= 0 and flat.max() < layout["n_total"]
    return out


def factors_of(layout, seed=0):
    """Per component: random Q_a (not orthogonal, not symmetric), positive lambda_a, and distinct masses."""
    rng = np.random.default_rng(seed)
    Q = [[rng.standard_normal((e, e)) for e in ext] for ext in layout["extents"]]
    lam = [[0.5 + rng.random(e) for e in ext] for ext in layout["extents"]]
    mass = [0.75 + 0.5 * c for c in range(len(layout["extents"]))]
    return Q, lam, mass


class Handle:
    def __init__(self, eng, layout, Q, lam, mass, only=None):
        pick = range(len(layout["extents"])) if only is None else [only]
        ext = [e for c in pick for e in layout["extents"][c]]
        d = len(layout["extents"][0])
        qs = [np.ascontiguousarray(q) for c in pick for q in Q[c]]
        ls = [np.ascontiguousarray(w) for c in pick for w in lam[c]]
        self.keep = qs + ls
        out = C.c_void_p()
        rc = eng.lib.nss_fdmc_create(len(pick), d, layout["n_total"], (C.c_int64 * len(pick))(*[layout["bases"][c] for c in pick]),
                                     layout["pitch"], (C.c_int64 * len(ext))(*ext),
                                     (C.c_void_p * len(qs))(*[q.ctypes.data for q in qs]),
                                     (C.c_void_p * len(ls))(*[w.ctypes.data for w in ls]),
                                     (C.c_double * len(pick))(*[mass[c] for c in pick]), C.byref(out))
        assert rc == 0 and out.value, eng.lib.nss_last_error()
        self.eng, self.ptr = eng, out

    def __del__(self):
        if self.ptr:
            self.eng.lib.nss_fdmc_destroy(self.ptr)
            self.ptr = None


def sums_of(lams):
    d = len(lams)
    out = lams[0].reshape((-1,) + (1,) * (d - 1))
    for a in range(1, d):
        out = out + lams[a].reshape((1,) * a + (-1,) + (1,) * (d - 1 - a))
    return out


def along(M, w, a):
    return np.moveaxis(np.tensordot(M, w, axes=(1, a)), 0, a)


def exact_solve(x, Q, lam, mass, sigma):
    """(the formula in long double, the chain of absolute values in double) for one component's array `x`."""
    mult = 1.0 / (LD(mass) + LD(sigma) * sums_of([w.astype(LD) for w in lam]))
    want, scale = x.astype(LD), np.abs(x)
    for a, q in enumerate(Q):
        want, scale = along(q.T.astype(LD), want, a), along(np.abs(q.T), scale, a)
    want, scale = want * mult, scale * np.asarray(np.abs(mult), dtype=np.float64)
    for a, q in enumerate(Q):
        want, scale = along(q.astype(LD), want, a), along(np.abs(q), scale, a)
    return want, scale


def guarded_output(eng, count):
    whole = eng.from_host(np.full(count + 2 * GUARD, SENT))
    return whole, eng.view(whole, GUARD, GUARD + count)


def check_guards(eng, whole, count):
    host = eng.to_host(whole)
    assert (host[:GUARD] == SENT).all() and (host[GUARD + count:] == SENT).all()


def solve(eng, handle, sigma, d_rhs, out):
    rc = eng.lib.nss_fdmc_solve_f64(handle.ptr, sigma, d_rhs.data_ptr(), out.data_ptr(), eng.stream)
    assert rc == 0, eng.lib.nss_last_error()
    eng.synchronize()
    return eng.to_host(out).copy()


# ---- 1. the kernel alone, synthetic handles -----------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(LAYOUTS))
def test_solve_on_synthetic_handles(hip_engine, name):
    eng, layout = hip_engine, LAYOUTS[name]
    ids, (Q, lam, mass) = ids_of(layout), factors_of(layout)
    n_total, sigma = layout["n_total"], 0.37
    rhs = np.random.default_rng(7).standard_normal(n_total)
    d_rhs = eng.from_host(rhs)
    whole, out = guarded_output(eng, n_total)
    batch = Handle(eng, layout, Q, lam, mass)
    first = solve(eng, batch, sigma, d_rhs, out)
    assert np.array_equal(eng.to_host(d_rhs), rhs)                       # rhs keeps its bits
    check_guards(eng, whole, n_total)
    outside = np.ones(n_total, dtype=bool)
    for c, g in enumerate(ids):
        outside[g.ravel()] = False
        want, scale = exact_solve(rhs[g], Q[c], lam[c], mass[c], sigma)
        err = np.abs(np.asarray(first[g].astype(LD) - want, dtype=np.float64))
        bound = (sum(2 * 2 * (e + 2) for e in g.shape) + 6) * U * scale
        print("%s component %d: max err / bound = %.3f" % (name, c, float((err / bound).max())))
        assert (err <= bound).all(), (c, np.argwhere(err > bound)[:8], float((err / bound).max()))
    assert (first[outside] == SENT).all()                                # no entry outside the components is written
    eng.upload(np.full(n_total, SENT), out)
    assert np.array_equal(solve(eng, batch, sigma, d_rhs, out), first)   # a second solve reproduces the first
    for c, g in enumerate(ids):                                          # ... and so does every component on its own
        eng.upload(np.full(n_total, SENT), out)
        alone = solve(eng, Handle(eng, layout, Q, lam, mass, only=c), sigma, d_rhs, out)
        assert np.array_equal(alone[g], first[g])
        mask = np.ones(n_total, dtype=bool)
        mask[g.ravel()] = False
        assert (alone[mask] == SENT).all()
    check_guards(eng, whole, n_total)


# ---- 2. one pass ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["mac3d_n5", "mac2d_n5"])
@pytest.mark.parametrize("transpose", [0, 1])
def test_pass_against_einsum(hip_engine, name, transpose):
    eng, layout = hip_engine, LAYOUTS[name]
    ids, (Q, lam, mass) = ids_of(layout), factors_of(layout, seed=1)
    n_total, dim = layout["n_total"], len(layout["extents"][0])
    handle = Handle(eng, layout, Q, lam, mass)
    src = np.random.default_rng(9).standard_normal(n_total)
    d_src = eng.from_host(src)
    whole, dst = guarded_output(eng, n_total)
    for axis in range(dim):
        for scaled, sigma in ((0, 0.0), (1, 0.05), (1, 3.0)):
            eng.upload(np.full(n_total, SENT), dst)
            rc = eng.lib.nss_fdmc_pass_f64(handle.ptr, axis, transpose, scaled, sigma, d_src.data_ptr(), dst.data_ptr(),
                                           eng.stream)
            assert rc == 0, eng.lib.nss_last_error()
            got = eng.to_host(dst).copy()
            outside = np.ones(n_total, dtype=bool)
            for c, g in enumerate(ids):
                outside[g.ravel()] = False
                M = Q[c][axis].T if transpose else Q[c][axis]
                want, scale = along(M.astype(LD), src[g].astype(LD), axis), along(np.abs(M), np.abs(src[g]), axis)
                n, extra = g.shape[axis], 4
                if scaled:
                    mult = 1.0 / (LD(mass[c]) + LD(sigma) * sums_of([w.astype(LD) for w in lam[c]]))
                    want, scale, extra = want * mult, scale * np.asarray(mult, dtype=np.float64), 10
                err = np.abs(np.asarray(got[g].astype(LD) - want, dtype=np.float64))
                bound = (2 * n + extra) * U * scale
                assert (err <= bound).all(), (axis, scaled, c, float((err / bound).max()))
            assert (got[outside] == SENT).all()
    assert np.array_equal(eng.to_host(d_src), src)
    check_guards(eng, whole, n_total)


# ---- 3. the refusals ------------------------------------------------------------------------------------------------------
def test_refusals(hip_engine):
    """Non-zero with a message, no handle, nothing launched (the output keeps its sentinel)."""
    eng, lib = hip_engine, hip_engine.lib
    layout = LAYOUTS["mac3d_n2"]
    Q, lam, mass = factors_of(layout)
    qs = [np.ascontiguousarray(q) for c in range(3) for q in Q[c]]
    ls = [np.ascontiguousarray(w) for c in range(3) for w in lam[c]]
    good = dict(ncomp=3, dim=3, n_total=layout["n_total"], base=(C.c_int64 * 3)(*layout["bases"]), pitch=layout["pitch"],
                ext=(C.c_int64 * 9)(*[e for ext in layout["extents"] for e in ext]),
                q=(C.c_void_p * 9)(*[q.ctypes.data for q in qs]), lam=(C.c_void_p * 9)(*[w.ctypes.data for w in ls]),
                mass=(C.c_double * 3)(*mass))
    out = C.c_void_p()

    def create(**change):
        a = dict(good, **change)
        return lib.nss_fdmc_create(a["ncomp"], a["dim"], a["n_total"], a["base"], a["pitch"], a["ext"], a["q"], a["lam"],
                                   a["mass"], a.get("out", C.byref(out)))
    assert create() == 0 and out.value                                    # (the arguments themselves are good)
    assert lib.nss_fdmc_destroy(out) == 0
    out = C.c_void_p()
    none9 = (C.c_void_p * 9)(*[None] * 9)
    bases = layout["bases"]
    bad = [dict(base=None), dict(ext=None), dict(q=None), dict(lam=None), dict(mass=None), dict(out=None), dict(q=none9),
           dict(lam=none9), dict(ncomp=0), dict(ncomp=4), dict(dim=1), dict(dim=4), dict(n_total=0), dict(n_total=2 ** 31),
           dict(pitch=0), dict(pitch=1),                                  # a slab of 2 entries every 1
           dict(pitch=3),                                                 # the slabs of components 0 and 1 collide
           dict(base=(C.c_int64 * 3)(bases[0], bases[0] + 1, bases[2])),  # component 1 on top of component 0
           dict(base=(C.c_int64 * 3)(bases[0], bases[1], bases[0] + layout["pitch"])),   # component 2 on slab 1 of component 0
           dict(n_total=layout["n_total"] - 1),                           # the last component past n_total
           dict(base=(C.c_int64 * 3)(-1, bases[1], bases[2])),
           dict(ext=(C.c_int64 * 9)(2, 2, 1, 2, 0, 2, 1, 2, 2)),
           dict(mass=(C.c_double * 3)(1.0, 0.0, 1.0)), dict(mass=(C.c_double * 3)(1.0, 1.0, -2.0)),
           dict(mass=(C.c_double * 3)(float("nan"), 1.0, 1.0))]
    for change in bad:
        assert create(**change) != 0, list(change)
        assert b"fdmc_create" in lib.nss_last_error() and not out.value, (list(change), lib.nss_last_error())
    handle = Handle(eng, layout, Q, lam, mass)
    d_rhs = eng.from_host(np.ones(layout["n_total"]))
    whole, dst = guarded_output(eng, layout["n_total"])
    r, o, h = d_rhs.data_ptr(), dst.data_ptr(), handle.ptr
    for args in [(None, 0.1, r, o), (h, 0.1, None, o), (h, 0.1, r, None), (h, 0.1, o, o), (h, -0.1, r, o),
                 (h, float("nan"), r, o), (h, float("inf"), r, o)]:
        assert lib.nss_fdmc_solve_f64(*args, eng.stream) != 0, args
        assert b"fdmc_solve" in lib.nss_last_error()
    for args in [(None, 0, 0, 0, 0.0, r, o), (h, 0, 0, 0, 0.0, None, o), (h, 0, 0, 0, 0.0, r, None), (h, 0, 0, 0, 0.0, o, o),
                 (h, -1, 0, 0, 0.0, r, o), (h, 3, 0, 0, 0.0, r, o), (h, 0, 0, 1, -1.0, r, o), (h, 0, 0, 1, float("nan"), r, o)]:
        assert lib.nss_fdmc_pass_f64(*args, eng.stream) != 0, args
        assert b"fdmc_pass" in lib.nss_last_error()
    eng.synchronize()
    assert (eng.to_host(whole) == SENT).all()
    assert lib.nss_fdmc_destroy(None) == 0


# ---- 4. the operators of the grid -------------------------------------------------------------------------------------------
OPERATORS = {"A2d_n2": ("A", 2, 2), "A2d_n12": ("A", 2, 12), "A2d_n33": ("A", 2, 33), "A3d_n2": ("A", 3, 2),
             "A3d_n7": ("A", 3, 7), "A3d_n17": ("A", 3, 17), "K2d_n12": ("K", 2, 12), "K3d_n7": ("K", 3, 7)}


@pytest.fixture(scope="module", params=sorted(OPERATORS))
def operator(request):
    from staggered_grid import mac_stokes
    kind, dim, n = OPERATORS[request.param]
    s = mac_stokes(dim, n, 0.01)
    if kind == "A":
        return request.param, s.A, s.component_ids, np.full(s.n_u, s.h ** s.dim)
    ops = s.scalar_operators(0.8, {"x-": 1.0, "x+": 0.0})
    return request.param, sp.csr_matrix(ops["K"]), [np.arange(s.n_p).reshape((n,) * dim)], np.asarray(ops["mass"], float)


@pytest.mark.parametrize("sigma", [0.05, 0.025])
def test_solve_against_the_operator(hip_engine, operator, sigma):
    import hipla
    eng = hip_engine
    name, mat, comps, mass = operator
    inv = hipla.ComponentFastDiagonalization(mat, comps, mass, sigma)
    assert inv.handle is not None and inv.iterations == 0 and inv.sigma == sigma
    n = mat.shape[0]
    op = (sp.diags(mass) + sigma * mat).tocsr()
    rhs = np.random.default_rng(3).standard_normal(n)
    size = np.linalg.norm(rhs)
    host = np.linalg.norm(op @ inv.factors.solve(rhs, sigma) - rhs) / size
    d_rhs = eng.from_host(rhs)
    whole, out = guarded_output(eng, n)
    assert inv.solve_resident(d_rhs, out) == 0
    first = eng.to_host(out).copy()
    res = np.linalg.norm(op @ first - rhs) / size
    print("%s sigma %g: residual %.3g (numpy restatement %.3g)" % (name, sigma, res, host))
    assert res <= max(10 * host, 1e-14)
    assert np.array_equal(eng.to_host(d_rhs), rhs)
    check_guards(eng, whole, n)
    eng.upload(np.full(n, SENT), out)
    assert inv.solve_resident(d_rhs, out, sigma) == 0                      # sigma by argument: the same launch
    assert np.array_equal(eng.to_host(out), first)
    x, y = hipla.Vector.from_numpy(rhs), hipla.Vector(n)                  # the protocol's statement reproduces it
    y.data = inv * x
    assert np.array_equal(y.numpy(), first) and np.array_equal(x.numpy(), rhs)
    x.data = inv * x                                                       # (x over itself: through a copy)
    assert np.array_equal(x.numpy(), first)
    other = 0.5 * sigma                                                    # the same handle at another sigma
    inv.sigma = other
    inv.solve_resident(d_rhs, out)
    op2 = (sp.diags(mass) + other * mat).tocsr()
    host2 = np.linalg.norm(op2 @ inv.factors.solve(rhs, other) - rhs) / size
    assert np.linalg.norm(op2 @ eng.to_host(out) - rhs) / size <= max(10 * host2, 1e-14)
