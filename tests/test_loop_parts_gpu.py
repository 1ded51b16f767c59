"""The partial-sum tree the CG and Lanczos loops share (`sum_partials_1024`, csrc/loop_parts.h) reads every partial once
and none twice: with a right-hand side of small integers every product and every partial sum of the device-started CG is
an integer far below 2^53 -- exact in fp64 in any order --, so <r, z> must come out as the integer itself.  The sizes put
1, 1024, 1025, 2049 and 1026 partials into the sum: one below and one above each trip count of its paired loop and of
its tail."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

pytestmark = pytest.mark.gpu

G_RZ = 0                                  # scal word of <r, z> at the start (csrc/cg.hip)
SIZES = [(1000, 1), (1024 * 1024, 1024), (1024 * 1025, 1025), (1024 * 2049, 2049), (1025 * 1024 + 1, 1026)]


@pytest.mark.parametrize("n,partials", SIZES)
def test_start_sum_is_exact_on_integers(hip_engine, n, partials):
    import hipla
    from hipla import fused
    eng = hip_engine
    A = hipla.SparseMatrix.from_scipy(sp.diags([-1.0, 2.5, -1.0], [-1, 0, 1], shape=(n, n), format="csr"))
    loop = fused.CgLoop.try_create(A, None)                 # no preconditioner: z = r, <r, z> = sum b^2
    assert loop is not None, fused.CgLoop.last_declined
    b = np.random.default_rng(1234).integers(-3, 4, size=n).astype(np.float64)
    want = float(int((b * b).sum()))
    d_b = eng.from_host(b)
    st = loop.state
    count_a, count_b = C.c_int64(), C.c_int64()
    eng._check(eng.lib.nss_cg_workspace(C.byref(st), C.byref(count_a), C.byref(count_b)))
    assert count_b.value == partials

    x = eng.zeros(n)
    loop.hist = eng.zeros(1)
    st.hist, st.x = loop.hist.data_ptr(), x.data_ptr()
    eng._check(eng.lib.nss_cg_start(C.byref(st), d_b.data_ptr(), 1e-10, eng.stream))
    got = float(eng.to_host(loop.scal)[G_RZ])
    print("n %d, %d partials: <r, z> %r, sum b^2 %r" % (n, partials, got, want))
    assert got == want

    runs = []
    for _ in range(3):                                      # the same through solve_resident, one iteration
        x = eng.zeros(n)
        assert loop.solve_resident(d_b, x, 1e-10, 1) == 1
        runs.append((eng.to_host(loop.hist)[:1].copy(), eng.to_host(loop.scal).copy(), eng.to_host(x).copy()))
    hist, scal, _ = runs[0]
    assert np.isfinite(hist[0]) and scal[G_RZ] == want
    for other in runs[1:]:
        for first, again in zip(runs[0], other):
            assert np.array_equal(first, again)
