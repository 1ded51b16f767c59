"""The vector layer underneath everything else, on the GPU: every kernel of csrc/blas1.hip through the product
engine's own entry points, at every branch point of its launch arithmetic and at every operand alignment, against
numpy (bit for bit on data where fp64 is exact) and against long double (element by element, inside the bound the
kernel's own operation count gives); then the expression layer of hipla/vector.py on views of one pool.

Scaffolding.  Every operand is a view pool[pad + off : pad + off + n] of ONE device buffer that was filled with a
sentinel bit pattern first (a NaN with a payload); off in {0, 1} per operand, independently, so that the all-aligned
form, the all-unaligned form and every mixed case that must fall back to 8-byte accesses are reached.  After each call
every byte outside the destination view must still be what it was: the odd tails of the 16-byte forms and the one-shot
triad grid are where a kernel would write one element too far.  Sizes: vector_reference.SIZES, with the arithmetic they
come from.  The clamp of the grid at NSS_MAX_STREAM_BLOCKS needs vectors above 5e8 bytes and is NOT tested here.

Which case names which export of blas1.hip that launches a kernel:
  nss_fill_f64            test_fill                       (HipEngine.fill)
  nss_lincomb_f64         test_lincomb_*                  (HipEngine.lincomb)
  nss_copy_f64            test_copy_and_scal_on_views     (HipEngine.copy)
  nss_scal_f64            test_copy_and_scal_on_views     (HipEngine.scal)
  nss_stream_triad_f64    test_stream_triad               (HipEngine.stream_triad)
  nss_diag_apply_f64      test_diag_apply                 (HipEngine.diag_apply)
  nss_reciprocal_f64      test_reciprocal                 (lib.nss_reciprocal_f64)
  nss_upwind_flux_f64     test_upwind_flux                (HipEngine.upwind_flux)
  nss_gather_f64          test_gather                     (HipEngine.gather)
  nss_dot_host_f64        test_dot_*                      (HipEngine.dot, HipEngine.dot_multi)
  nss_dot_f64             test_dot_*                      (lib.nss_dot_f64, the device result)
Which case reaches which template instantiation (the 16-byte form VEC2 = true is taken when EVERY pointer of the call
is 16-byte aligned, i.e. all offsets 0; any offset 1 gives VEC2 = false):
  fill_kernel<VEC2>           test_fill, off = 0 / 1
  lincomb_kernel<NT, VEC2>    test_lincomb_every_alignment, nt = NT = 1 .. 4, offsets all 0 / any 1  (8 instantiations)
  triad_kernel<VEC2>          test_stream_triad, offsets all 0 / any 1
  diag_kernel<VEC2, BETA>     test_diag_apply: beta == 0 -> BETA = false, beta != 0 -> BETA = true, each with offsets
                              all 0 / any 1                                                           (4 instantiations)
  dot_partial_kernel          vec2 per pair: test_dot_one_pair at offsets (0, 0) / the three others"""

import ctypes as C
import itertools

import numpy as np
import pytest

import vector_reference as vr
from vector_reference import LD, U, gamma

pytestmark = pytest.mark.gpu

PAD = 8                                                     # canary elements on either side of every view (even)
SENTINEL = 0x7FF4C0DEC0DE1234                               # a NaN nobody computes
OFFSETS = (0, 1)


class Arena:
    """One device buffer cut into slots of the given lengths; a view of slot k starts PAD + off elements into it."""

    def __init__(self, eng, lengths):
        self.eng = eng
        self.sizes = [(m + 2 * PAD + 2 + 1) & ~1 for m in lengths]          # even: every slot starts 16-byte aligned
        self.start = np.concatenate([[0], np.cumsum(self.sizes)]).astype(np.int64)
        self.lengths = list(lengths)
        self.host = np.empty(int(self.start[-1]), dtype=np.float64)
        self.dev = eng.empty(self.host.size)
        assert self.dev.data_ptr() % 16 == 0
        self.reset()

    def reset(self):
        self.host.view(np.int64)[:] = SENTINEL

    def span(self, k, off, m=None):
        a = int(self.start[k]) + PAD + off
        return a, a + (self.lengths[k] if m is None else m)

    def put(self, k, off, data):
        a, b = self.span(k, off, len(data))
        assert b + PAD <= self.start[k + 1]
        self.host[a:b] = data
        return a, b

    def upload(self):
        self.eng.upload(self.host, self.dev)

    def view(self, span):
        v = self.eng.view(self.dev, *span)
        assert v.shape[0] == 0 or v.data_ptr() % 16 == 8 * (span[0] & 1)     # the alignment the case is about
        return v

    def after(self, dest):
        """The destination view after the call; everything outside it must be bit-identical to what was uploaded."""
        got = self.eng.to_host(self.dev)
        keep = np.ones(got.size, dtype=bool)
        keep[dest[0]:dest[1]] = False
        moved = np.nonzero((vr.bits(got) != vr.bits(self.host)) & keep)[0]
        assert moved.size == 0, "elements outside the destination [%d, %d) changed: %s" % (dest[0], dest[1], moved[:8])
        return got[dest[0]:dest[1]]


def same_bits(got, want, what):
    bad = np.nonzero(vr.bits(got) != vr.bits(want))[0]
    assert bad.size == 0, "%s: %d elements differ, first at %d: %r vs %r" % (
        what, bad.size, bad[0], got[bad[0]], want[bad[0]])


def same_values(got, want, what):
    """Exact values (the statements of the expression layer fix no order of the terms, so not the sign of a zero)."""
    bad = np.nonzero(~(np.asarray(got) == np.asarray(want)))[0]
    assert bad.size == 0, "%s: %d elements differ, first at %d: %r vs %r" % (
        what, bad.size, bad[0], got[bad[0]], want[bad[0]])


def inside(got, ref, bound, what):
    err = np.abs(got.astype(LD) - ref)
    bad = np.nonzero(~(err <= bound))[0]                     # (a NaN is outside every bound)
    assert bad.size == 0, "%s: %d elements outside the bound, first at %d: error %.3e, bound %.3e" % (
        what, bad.size, bad[0], float(err[bad[0]]), float(bound[bad[0]]))


# ---- fill ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", vr.SIZES)
def test_fill(hip_engine, n):
    arena = Arena(hip_engine, [n])
    for off, value in itertools.product(OFFSETS, (3.5, -0.0)):
        arena.reset()
        dst = arena.span(0, off)
        arena.upload()
        hip_engine.fill(arena.view(dst), value)
        same_bits(arena.after(dst), np.full(n, value), "fill off=%d" % off)


# ---- lincomb -------------------------------------------------------------------------------------------------------
EXACT_COEF = (2.0, -1.0, 3.0, -2.0)
REAL_COEF = (0.7310585786300049, -1.3, 2.718281828459045, -1.0 / 3.0)


def _lincomb_values(pattern, coef, data):
    """(numpy evaluation in the kernel's order, long double value, bound): one product and nt - 1 fmas are nt
    roundings of partial sums of the c_t x_t, so |error| <= nt u / (1 - nt u) * sum |c_t x_t| (gamma(nt))."""
    r = coef[0] * data[pattern[0]]
    ref = LD(coef[0]) * data[pattern[0]].astype(LD)
    absum = np.abs(ref)
    for c, k in zip(coef[1:], pattern[1:]):
        r = r + c * data[k]
        ref = ref + LD(c) * data[k].astype(LD)
        absum = absum + np.abs(LD(c) * data[k].astype(LD))
    return r, ref, gamma(len(pattern)) * absum.astype(np.float64)


def _lincomb_cases(eng, n, patterns):
    """Every pattern (slot of each term; slot 0 is the destination) at every combination of offsets, once on small
    integers (exact) and once on reals (rounding bound)."""
    arena = Arena(eng, [n] * 5)
    rng = np.random.default_rng(n)
    for exact in (True, False):
        data = {k: (vr.small_ints(rng, n) if exact else vr.spread(rng, n)) for k in range(5)}
        coef_all = EXACT_COEF if exact else REAL_COEF
        for pattern in patterns:
            coef = coef_all[:len(pattern)]
            want, ref, bound = _lincomb_values(pattern, coef, data)
            slots = sorted(set(pattern) | {0})
            for offs in itertools.product(OFFSETS, repeat=len(slots)):
                off = dict(zip(slots, offs))
                arena.reset()
                spans = {k: (arena.put(k, off[k], data[k]) if k in pattern else arena.span(k, off[k])) for k in slots}
                arena.upload()
                eng.lincomb(arena.view(spans[0]), [(c, arena.view(spans[k])) for c, k in zip(coef, pattern)])
                got = arena.after(spans[0])
                what = "lincomb terms=%s offsets=%s" % (pattern, off)
                if exact:
                    same_bits(got, want, what)
                else:
                    inside(got, ref, bound, what)


@pytest.mark.parametrize("n", vr.SIZES)
def test_lincomb_every_alignment(hip_engine, n):
    _lincomb_cases(hip_engine, n, [(1,), (1, 2), (1, 2, 3), (1, 2, 3, 4)])


@pytest.mark.parametrize("n", vr.SIZES)
def test_lincomb_destination_among_operands(hip_engine, n):
    """The kernel takes no __restrict__: the destination as the first, a middle and the last operand, as two operands
    at once, and as every operand (x = a x + b x ...)."""
    _lincomb_cases(hip_engine, n, [(0, 1, 2, 3), (1, 0, 2, 3), (1, 2, 0, 3), (1, 2, 3, 0), (0, 1), (1, 0), (0, 1, 0, 2),
                                   (1, 0, 2, 0), (0,), (0, 0), (0, 0, 0), (0, 0, 0, 0)])


@pytest.mark.parametrize("n", vr.SIZES)
def test_copy_and_scal_on_views(hip_engine, n):
    arena = Arena(hip_engine, [n, n])
    rng = np.random.default_rng(n)
    x, k = vr.spread(rng, n), vr.small_ints(rng, n)
    for od, ox in itertools.product(OFFSETS, OFFSETS):
        arena.reset()
        dst, src = arena.span(0, od), arena.put(1, ox, x)
        arena.upload()
        hip_engine.copy(arena.view(src), arena.view(dst))
        same_bits(arena.after(dst), x, "copy offsets=%d,%d" % (od, ox))             # 1.0 * x is x
    for od in OFFSETS:
        for data, a in ((k, -3.0), (x, REAL_COEF[0])):
            arena.reset()
            dst = arena.put(0, od, data)
            arena.upload()
            hip_engine.scal(arena.view(dst), a)
            got = arena.after(dst)
            if data is k:
                same_bits(got, a * k, "scal off=%d" % od)
            else:                                                                    # one product: one rounding
                inside(got, LD(a) * x.astype(LD), gamma(1) * np.abs(a * x), "scal off=%d" % od)


# ---- STREAM triad --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", vr.SIZES)
def test_stream_triad(hip_engine, n):
    """z = fma(a, y, x): ONE rounding of the exact value, so |error| <= u |x + a y| -- a bound that shrinks with
    cancellation, hence the reference forms a y exactly (two_product) before it adds in long double."""
    arena = Arena(hip_engine, [n, n, n])
    rng = np.random.default_rng(n)
    for exact in (True, False):
        x, y = (vr.small_ints(rng, n), vr.small_ints(rng, n)) if exact else (vr.spread(rng, n), vr.spread(rng, n))
        a = -3.0 if exact else REAL_COEF[2]
        p, e = vr.two_product(a, y)
        ref = (x.astype(LD) + p.astype(LD)) + e.astype(LD)
        for oz, ox, oy in itertools.product(OFFSETS, repeat=3):
            arena.reset()
            dst, sx, sy = arena.span(0, oz), arena.put(1, ox, x), arena.put(2, oy, y)
            arena.upload()
            hip_engine.stream_triad(a, arena.view(sx), arena.view(sy), arena.view(dst))
            got = arena.after(dst)
            what = "triad offsets z,x,y=%d,%d,%d" % (oz, ox, oy)
            if exact:
                same_bits(got, x + a * y, what)
            else:
                inside(got, ref, U * np.abs(ref).astype(np.float64), what)


# ---- diagonal scale ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", vr.SIZES)
def test_diag_apply(hip_engine, n):
    """y = alpha * (d * x) (two roundings), then fma(beta, y, .) (a third): |error| <= 3 u (|alpha d x| + |beta y|).
    beta == 0 must not read y: it is pre-filled with NaN and no NaN may survive.  beta != 0: plain and y is x."""
    eng = hip_engine
    arena = Arena(eng, [n, n, n])
    rng = np.random.default_rng(n)
    for exact in (True, False):
        d, x, y = ((vr.small_ints(rng, n) for _ in range(3)) if exact else (vr.spread(rng, n) for _ in range(3)))
        alpha, beta = (-2.0, 3.0) if exact else (REAL_COEF[0], REAL_COEF[1])
        for mode in ("beta=0", "plain", "y is x"):
            yy = np.full(n, np.nan) if mode == "beta=0" else y
            xx = yy if mode == "y is x" else x
            b = 0.0 if mode == "beta=0" else beta
            want = alpha * (d * xx)
            ref = LD(alpha) * (d.astype(LD) * xx.astype(LD))
            absum = np.abs(ref)
            if b != 0.0:
                want = want + b * yy
                ref = ref + LD(b) * yy.astype(LD)
                absum = absum + np.abs(LD(b) * yy.astype(LD))
            bound = 3.0 * U * absum.astype(np.float64)
            for oy, od, ox in itertools.product(OFFSETS, OFFSETS, OFFSETS if mode != "y is x" else (0,)):
                arena.reset()
                sy, sd = arena.put(0, oy, yy), arena.put(1, od, d)
                sx = sy if mode == "y is x" else arena.put(2, ox, x)
                arena.upload()
                eng.diag_apply(arena.view(sd), alpha, arena.view(sx), b, arena.view(sy))
                got = arena.after(sy)
                what = "diag_apply %s offsets y,d,x=%d,%d,%d" % (mode, oy, od, ox)
                assert not np.isnan(got).any(), what
                if exact:
                    same_bits(got, want, what)
                else:
                    inside(got, ref, bound, what)


# ---- reciprocal ----------------------------------------------------------------------------------------------------
def _reciprocal_inputs(rng):
    tiny, huge = np.finfo(np.float64).tiny, np.finfo(np.float64).max
    special = np.array([1.0, -3.0, 0.0, -0.0, np.inf, -np.inf, np.nan, huge, -huge, tiny, -tiny, 5e-324, -5e-324,
                        tiny / 3.0, -tiny / 1024.0, 2.0 ** -1022 * (1 - 2.0 ** -52), 4.0 / huge, 7.0, 1e308, 3e-308])
    sub = rng.integers(1, 1 << 52, 64).astype(np.int64).view(np.float64)      # subnormals of every size
    return np.concatenate([special, sub, vr.spread(rng, 4100)])


@pytest.mark.parametrize("n", vr.SIZES)
def test_reciprocal(hip_engine, n):
    """The build has no fast-math flag: fp64 division is IEEE, so 1 / x must be numpy's 1.0 / x bit for bit (NaN
    matches NaN) -- normal values, subnormals, the largest finite value, +-0, +-inf, NaN; in place (the only caller:
    the inverse of a diagonal) and out of place."""
    eng = hip_engine
    arena = Arena(eng, [n, n])
    base = _reciprocal_inputs(np.random.default_rng(7))
    for rot in (0, 6, 13):
        x = np.roll(base, -rot)[:n]                          # (so that n = 1, 2, 3 see more than the first values)
        with np.errstate(divide="ignore", over="ignore", under="ignore", invalid="ignore"):
            want = 1.0 / x
        for in_place, oy, ox in itertools.product((True, False), OFFSETS, OFFSETS):
            if in_place and ox != oy:
                continue
            arena.reset()
            sx = arena.put(1, ox, x) if not in_place else None
            sy = arena.put(0, oy, x) if in_place else arena.span(0, oy)
            arena.upload()
            src = arena.view(sy if in_place else sx)
            dst = arena.view(sy)
            eng._check(eng.lib.nss_reciprocal_f64(n, src.data_ptr(), dst.data_ptr(), eng.stream))
            got = arena.after(sy)
            what = "reciprocal %s offsets y,x=%d,%d" % ("in place" if in_place else "out of place", oy, ox)
            assert np.array_equal(np.isnan(got), np.isnan(want)), what
            ok = ~np.isnan(want)
            same_bits(got[ok], want[ok], what)


# ---- donor-cell flux -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", vr.SIZES)
def test_upwind_flux(hip_engine, n):
    """f = fma(a, avg, -(|a| diff) / 2): the product |a| diff rounds once (halving is exact), the fma once:
    |error| <= 2 u (|a avg| + |a diff| / 2).  Exact data (even diff): numpy's value bit for bit, and the donor-cell
    identity a (avg - diff / 2) for a > 0, a (avg + diff / 2) for a < 0."""
    eng = hip_engine
    arena = Arena(eng, [n] * 4)
    rng = np.random.default_rng(n)
    for exact in (True, False):
        if exact:
            adv, avg, diff = vr.small_ints(rng, n), vr.small_ints(rng, n), 2.0 * vr.small_ints(rng, n)
            adv[::7] = 0.0
            adv[3::7] = -0.0
        else:
            adv, avg, diff = vr.spread(rng, n), vr.spread(rng, n), vr.spread(rng, n)
        want = adv * avg - 0.5 * (np.abs(adv) * diff)
        ref = adv.astype(LD) * avg.astype(LD) - LD(0.5) * (np.abs(adv).astype(LD) * diff.astype(LD))
        bound = 2.0 * U * (np.abs(adv.astype(LD) * avg.astype(LD))
                           + LD(0.5) * np.abs(adv.astype(LD) * diff.astype(LD))).astype(np.float64)
        for offs in itertools.product(OFFSETS, repeat=4):
            arena.reset()
            dst = arena.span(0, offs[0])
            sa, sv, sd = arena.put(1, offs[1], adv), arena.put(2, offs[2], avg), arena.put(3, offs[3], diff)
            arena.upload()
            eng.upwind_flux(arena.view(sa), arena.view(sv), arena.view(sd), arena.view(dst))
            got = arena.after(dst)
            what = "upwind_flux offsets f,adv,avg,diff=%s" % (offs,)
            if exact:
                same_bits(got, want, what)
                up, down = adv > 0, adv < 0
                assert np.array_equal(got[up], adv[up] * (avg[up] - diff[up] / 2)), what
                assert np.array_equal(got[down], adv[down] * (avg[down] + diff[down] / 2)), what
                assert not got[adv == 0].any(), what
            else:
                inside(got, ref, bound, what)


# ---- gather --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 255, 256, 257, 70001])
def test_gather(hip_engine, n):
    """dst[i] = src[idx[i]] exactly; the source is longer than the destination, the indices repeat and include 0 and
    the last element of the source."""
    eng = hip_engine
    m = n + 37
    arena = Arena(eng, [n, m])
    rng = np.random.default_rng(n)
    src = vr.spread(rng, m)
    for variant in range(2):
        idx = rng.integers(0, m, n).astype(np.int32)
        if n == 1:
            idx[0] = (0, m - 1)[variant]
        else:
            idx[0], idx[-1] = ((0, m - 1), (m - 1, 0))[variant]
            idx[n // 2] = idx[n // 3]                        # repeats
            idx[1] = idx[0]
        assert idx.min() >= 0 and idx.max() < m
        didx = eng.index_buffer(idx)
        for od, osrc in itertools.product(OFFSETS, OFFSETS):
            arena.reset()
            dst, ss = arena.span(0, od), arena.put(1, osrc, src)
            arena.upload()
            eng.gather(didx, arena.view(ss), arena.view(dst))
            same_bits(arena.after(dst), src[idx], "gather offsets dst,src=%d,%d" % (od, osrc))
            assert np.array_equal(eng.index_to_host(didx), idx)


# ---- dot -----------------------------------------------------------------------------------------------------------
def _dot_args(views):
    k = len(views)
    return (k, (C.c_int64 * k)(*[x.shape[0] for x, _ in views]), (C.c_void_p * k)(*[x.data_ptr() for x, _ in views]),
            (C.c_void_p * k)(*[y.data_ptr() for _, y in views]))


def _dot_launch(eng, arena, lengths, offsets, data):
    """One launch of launch_dot over the pairs (slot 2 p, slot 2 p + 1): the value of five calls of nss_dot_host_f64
    (through HipEngine.dot_multi), which must agree to the bit with each other and with nss_dot_f64's device result."""
    arena.reset()
    views = []
    for p, (m, (ox, oy)) in enumerate(zip(lengths, offsets)):
        sx, sy = arena.put(2 * p, ox, data[p][0]), arena.put(2 * p + 1, oy, data[p][1])
        views.append((arena.view(sx), arena.view(sy)))
    arena.upload()
    values = [eng.dot_multi(views) for _ in range(5)]
    result = eng.empty(1)
    eng._check(eng.lib.nss_dot_f64(*_dot_args(views), result.data_ptr(), eng.stream))
    values.append(float(eng.to_host(result)[0]))
    assert len({np.float64(v).view(np.int64).item() for v in values}) == 1, values
    return values[0]


def _dot_case(eng, lengths, offsets, rng):
    """The exact integer on integer data; on reals |error| <= gamma(D) sum |x_i y_i|.

    D, the longest chain of roundings a product passes through, from the layout of launch_dot and its two kernels
    (vector_reference.dot_depth).  A pair of length n gets B = min(max(ceil(n / 2048), 1), 32768) workgroups of 256
    lanes; a lane takes the items i, i + 256 B, ... -- elements, or double2's (n >> 1 of them) when both pointers are
    16-byte aligned.
      * the per-lane chain acc = fma(x, y, acc): the lane's first product is rounded in every one of its T trips,
        T = ceil(items / (256 B)) for lane 0 of workgroup 0, the busiest; in the 16-byte form that lane adds the odd
        tail after its loop: T + 1                                                          T (+ 1) roundings
      * acc0 + acc1 (exact in the 8-byte form, where acc1 stays 0; counted all the same)    1
      * the wave butterfly over 64 lanes                                                    6
      * the block sum lds[0] + lds[1] + lds[2] + lds[3]                                     3
      * dot_final_kernel: lane t adds the partials t, t + 256, ... of ALL pairs of the launch, the first onto 0.0
        (exact): ceil(partials / 256) - 1                                                   L - 1
      * its butterfly and block sum                                                         6 + 3
    Each rounding multiplies what it rounds by (1 + delta), |delta| <= u; a product picks up at most D such factors,
    and prod (1 + delta) - 1 is at most gamma(D) = D u / (1 - D u) in magnitude."""
    arena = Arena(eng, [m for m in lengths for _ in range(2)])
    ints = [(vr.small_ints(rng, m), vr.small_ints(rng, m)) for m in lengths]
    got = _dot_launch(eng, arena, lengths, offsets, ints)
    assert got == float(sum(int(np.dot(x.astype(np.int64), y.astype(np.int64))) for x, y in ints)), (lengths, offsets)
    reals = [(vr.spread(rng, m), vr.spread(rng, m)) for m in lengths]
    got = _dot_launch(eng, arena, lengths, offsets, reals)
    ref, absum = vr.dot_reference(reals)
    depth = vr.dot_depth([(m, ox == 0 and oy == 0) for m, (ox, oy) in zip(lengths, offsets)])
    err, bound = abs(LD(got) - ref), gamma(depth) * absum
    assert err <= bound, "dot lengths=%s offsets=%s: error %.3e, bound %.3e (D = %d)" % (
        lengths, offsets, float(err), bound, depth)


@pytest.mark.parametrize("n", vr.SIZES + (vr.DOT_TWO_TRIPS,))
def test_dot_one_pair(hip_engine, n):
    rng = np.random.default_rng(n)
    for offsets in itertools.product(OFFSETS, OFFSETS):
        _dot_case(hip_engine, [n], [offsets], rng)


@pytest.mark.parametrize("lengths", [(0,), (0, 1), (1, 4097, 0), (2049, 0, 1, 513), (257, 2048, 3, 1025),
                                     (4097, 2047, 255, 512), (1023, 1024), (2, 511, 256)],
                         ids=lambda t: "-".join(map(str, t)))
def test_dot_several_pairs(hip_engine, lengths):
    """1 to 4 pairs in one launch, alignment mixed per pair (all aligned, all unaligned, then three seeded draws)."""
    rng = np.random.default_rng(len(lengths) + sum(lengths))
    draws = [[(0, 0)] * len(lengths), [(1, 1)] * len(lengths)]
    draws += [[tuple(int(o) for o in rng.integers(0, 2, 2)) for _ in lengths] for _ in range(3)]
    for offsets in draws:
        _dot_case(hip_engine, list(lengths), offsets, rng)


@pytest.mark.parametrize("npairs", [5, 8, 9])
def test_dot_multi_chunks(hip_engine, npairs):
    """HipEngine.dot_multi launches chunks of four pairs (4 + 1, 4 + 4, 4 + 4 + 1) and adds the chunk values on the
    host, the first onto 0.0: chunks - 1 more roundings on top of the deepest chunk."""
    eng = hip_engine
    rng = np.random.default_rng(npairs)
    lengths = [257, 0, 2049, 1, 1024, 513, 4097, 3, 2047][:npairs]
    offsets = [tuple(int(o) for o in rng.integers(0, 2, 2)) for _ in lengths]
    arena = Arena(eng, [m for m in lengths for _ in range(2)])
    for exact in (True, False):
        data = [((vr.small_ints(rng, m), vr.small_ints(rng, m)) if exact else (vr.spread(rng, m), vr.spread(rng, m)))
                for m in lengths]
        arena.reset()
        views = []
        for p, (ox, oy) in enumerate(offsets):
            sx, sy = arena.put(2 * p, ox, data[p][0]), arena.put(2 * p + 1, oy, data[p][1])
            views.append((arena.view(sx), arena.view(sy)))
        arena.upload()
        values = {eng.dot_multi(views) for _ in range(5)}
        assert len(values) == 1
        got = values.pop()
        if exact:
            assert got == float(sum(int(np.dot(x.astype(np.int64), y.astype(np.int64))) for x, y in data))
            continue
        ref, absum = vr.dot_reference(data)
        aligned = [(m, ox == 0 and oy == 0) for m, (ox, oy) in zip(lengths, offsets)]
        chunks = [aligned[k:k + 4] for k in range(0, npairs, 4)]
        depth = max(vr.dot_depth(c) for c in chunks) + len(chunks) - 1
        err, bound = abs(LD(got) - ref), gamma(depth) * absum
        assert err <= bound, "dot_multi %d pairs: error %.3e, bound %.3e (D = %d)" % (npairs, float(err), bound, depth)


def test_dot_multi_refuses_mismatching_lengths(hip_engine):
    """The kernel takes each length from x alone: the refusal comes from the host, nothing is launched."""
    import hipla
    a = hipla.BlockVector([hipla.Vector(8), hipla.Vector(5)])
    b = hipla.BlockVector([hipla.Vector(8), hipla.Vector(4)])
    with pytest.raises(ValueError):
        hipla.InnerProduct(a, b)
    with pytest.raises(ValueError):
        hip_engine.dot_multi([(a[0].buf, b[0].buf), (a[1].buf, b[1].buf)])
    with pytest.raises(ValueError):
        hip_engine.dot(a[1].buf, b[1].buf)


# ---- the expression layer on the product engine --------------------------------------------------------------------
class Launches:
    """Counts the roundings of every launch a statement decomposes into, and holds lincomb to the aliasing rule."""

    def __init__(self, eng, monkeypatch):
        self.roundings = []
        self.longest_row = 0                                 # of the matrix the current statement uses
        lincomb, scal, spmv = eng.lincomb, eng.scal, eng.csr_spmv

        def spy_lincomb(dst, terms):
            for _, b in terms:
                assert eng.same_buffer(dst, b) or not eng.overlaps(dst, b), "operand overlaps the destination"
            self.roundings.append(len(terms))                # one product, nt - 1 fmas
            lincomb(dst, terms)

        def spy_scal(buf, a):
            self.roundings.append(1)
            scal(buf, a)

        def spy_spmv(h, alpha, x, beta, y):
            # a row of r entries: r roundings of its products' partial sums, at most six more where a butterfly joins
            # the lanes that share a row, one for alpha and one for the beta fma
            self.roundings.append(self.longest_row + 6 + 2)
            spmv(h, alpha, x, beta, y)

        monkeypatch.setattr(eng, "lincomb", spy_lincomb, raising=False)
        monkeypatch.setattr(eng, "scal", spy_scal, raising=False)
        monkeypatch.setattr(eng, "csr_spmv", spy_spmv, raising=False)

    def take(self):
        r, self.roundings = self.roundings, []
        return r


def test_random_statements_on_views(hip_engine, monkeypatch):
    """80 seeded statements (=, +=, -=; 1 to 7 terms, plain or M * v) on views at odd and even offsets of one pool,
    the destination aliased exactly, partly or not at all, against the long double evaluation with the right-hand side
    formed first.  The bound is the sum of the bounds of the launches the statement decomposed into (recorded while it
    ran): a launch with k roundings errs by at most gamma(k) times the sum of the magnitudes it combines, and every
    such sum is at most S (1 + gamma(k)) with S = sum |c| |x| + sum |c| (|M| |x|) (+ |old destination|) of the whole
    statement -- the second-order factor is the 1 + 2^-40 below."""
    import hipla
    eng = hip_engine
    rng = np.random.default_rng(80)
    mats = {}
    for n in vr.STATEMENT_SIZES:
        m, _, longest = vr.statement_matrix(n)
        mats[n] = (hipla.SparseMatrix.from_scipy(m), longest)
    record = Launches(eng, monkeypatch)
    seen = set()
    for k in range(80):
        n = vr.STATEMENT_SIZES[k % len(vr.STATEMENT_SIZES)]
        M, longest = mats[n]
        pool = vr.spread(rng, vr.pool_length(n))
        P = hipla.Vector.from_numpy(pool)
        assert P.buf.data_ptr() % 16 == 0
        statement = vr.random_statement(rng, n)
        record.take()
        record.longest_row = longest
        vr.run_statement(P, M, n, statement)
        roundings = record.take()
        ref, S = vr.statement_reference(pool, n, statement)
        dest = statement[1]
        got = P.numpy()
        bound = sum(gamma(r) for r in roundings) * (1.0 + 2.0 ** -40) * S
        inside(got[dest:dest + n], ref, bound, "statement %d %r" % (k, statement))
        want = pool.copy()
        want[dest:dest + n] = got[dest:dest + n]
        same_bits(got, want, "outside the destination, statement %d %r" % (k, statement))
        seen.add((statement[0], dest & 1))
    assert len(seen) == 6, seen                              # every operator at an odd and an even destination


@pytest.mark.parametrize("shift", vr.OVERLAP_SHIFTS)
def test_partly_overlapping_operands(hip_engine, shift):
    """x[s:n] = x[0:n-s] and its kin, both directions: the numpy value (right-hand side first) on integer data, exactly,
    three times over with the same bits."""
    import hipla
    n = vr.OVERLAP_N
    rng = np.random.default_rng(shift)
    x0, y0 = vr.small_ints(rng, n), vr.small_ints(rng, n)
    for name, run, ref in vr.overlap_statements(n, shift):
        x, y = x0.copy(), y0.copy()
        ref(x, y)
        runs = set()
        for _ in range(3):
            X, Y = hipla.Vector.from_numpy(x0), hipla.Vector.from_numpy(y0)
            run(X, Y)
            same_values(X.numpy(), x, name)
            same_values(Y.numpy(), y0, name)
            runs.add(X.numpy().tobytes())
        assert len(runs) == 1, name


@pytest.mark.parametrize("sizes", [(0,), (513,), (257, 0, 1025, 3), (512, 1, 0, 2049, 64),
                                   (255, 3, 1024, 0, 1, 2047, 513, 2, 4097)], ids=lambda t: "-".join(map(str, t)))
def test_block_vectors(hip_engine, sizes):
    """1, 4, 5 and 9 components, one of length 0: assignment, accumulation and scaling component by component (exact
    on integers); InnerProduct and Norm against long double with the dot's bound -- chunks of four components, each
    component in storage of its own (16-byte aligned), the chunk values added on the host."""
    import hipla
    rng = np.random.default_rng(len(sizes))
    a, b, c = ([vr.small_ints(rng, m) for m in sizes] for _ in range(3))

    def block(parts):
        return hipla.BlockVector([hipla.Vector.from_numpy(v) for v in parts])

    A, B, Cv = block(a), block(b), block(c)
    Cv.data = 2.0 * A - B
    cat = np.concatenate
    same_values(Cv.numpy(), cat([2.0 * x - y for x, y in zip(a, b)]), "block assignment")
    Cv.data += 3.0 * A
    same_values(Cv.numpy(), cat([5.0 * x - y for x, y in zip(a, b)]), "block accumulation")
    Cv.data -= Cv + B
    same_values(Cv.numpy(), cat([-y for y in b]), "block accumulation of itself")
    Cv *= -3.0
    same_values(Cv.numpy(), cat([3.0 * y for y in b]), "block scaling")
    Cv[:] = 1.5
    same_values(Cv.numpy(), np.full(sum(sizes), 1.5), "block fill")
    assert hipla.InnerProduct(A, B) == float(sum(int(np.dot(x.astype(np.int64), y.astype(np.int64)))
                                                 for x, y in zip(a, b)))
    x, y = [vr.spread(rng, m) for m in sizes], [vr.spread(rng, m) for m in sizes]
    X, Y = block(x), block(y)
    assert all(v.buf.shape[0] == 0 or v.buf.data_ptr() % 16 == 0 for v in X.components + Y.components)
    chunks = [[(m, True) for m in sizes[k:k + 4]] for k in range(0, len(sizes), 4)]
    depth = max(vr.dot_depth(ch) for ch in chunks) + len(chunks) - 1
    ref, absum = vr.dot_reference(list(zip(x, y)))
    got = hipla.InnerProduct(X, Y)
    assert abs(LD(got) - ref) <= gamma(depth) * absum, (float(abs(LD(got) - ref)), gamma(depth) * absum)
    ref2, _ = vr.dot_reference(list(zip(x, x)))
    # sqrt(s (1 + d)) = sqrt(s) (1 + e) with |e| <= |d| <= gamma(D) (all products positive), then sqrt's own rounding
    want = np.sqrt(ref2)
    assert abs(LD(hipla.Norm(X)) - want) <= want * (gamma(depth) + U) * (1.0 + U)
    assert abs(LD(X.Norm()) - want) <= want * (gamma(depth) + U) * (1.0 + U)
