"""`hipla.fdm.gather_factors` where there is no device: it reads a matrix that is resident on the
HIP engine, and says so of anything else; nothing falls back to the host behind the caller's back."""

import numpy as np
import pytest
import scipy.sparse as sp


def test_gather_factors_needs_the_hip_engine_and_a_resident_matrix(numpy_engine):
    import hipla
    from hipla import fdm
    from staggered_grid import mac_stokes
    s = mac_stokes(2, 5, 0.01)
    components = [np.asarray(g, dtype=np.int64) for g in s.component_ids]
    bases, pitch = fdm._affine_layout(components, s.n_u)
    shapes = [g.shape for g in components]
    assert not fdm.gather_available(numpy_engine)
    with pytest.raises(ValueError, match="nss_fdm_gather_factors"):
        fdm.gather_factors(hipla.SparseMatrix.from_scipy(s.A), bases, pitch, shapes)
    with pytest.raises(ValueError, match="SparseMatrix"):
        fdm.gather_factors(sp.csr_matrix(s.A), bases, pitch, shapes)
    # the host path is what it was: the factors still come from fdm_factors
    made, why = fdm.inverse_factors(s.A, s.component_ids)
    assert why is None and [f.extents for f in made.factors] == shapes


def test_the_entry_point_is_no_setter():
    """It takes pointers: the table of the process-wide overrides (tests/test_overrides_cpu.py) does not see it."""
    import ctypes
    from hipla import hip_engine as he
    _, args = he._signatures()["nss_fdm_gather_factors"]
    assert len(args) == 9 and not all(a in (ctypes.c_int32, ctypes.c_int64) for a in args)
