"""The process-wide plan overrides (hipla/hip_engine.py: OVERRIDES, overrides(), reset_overrides()) on a CPU-only box:
the setters and nss_csr_value_codes_wanted are host code.  The library has no getters; what is observable is
nss_csr_value_codes_wanted(1000 rows) -- 0 by the size rule, 1 under value_codes=1 -- and the module's record of the
arguments in force."""

import ctypes
import functools
import os

import pytest

from hipla import hip_engine as he


@pytest.fixture
def lib(monkeypatch):
    """the library with every switch at its default and no variable of the table set; defaults again afterwards"""
    import __graft_entry__ as entry
    if not os.path.exists(he.LIB_PATH):
        entry.build()
    for o in he.OVERRIDES.values():
        for var in o.env:
            monkeypatch.delenv(var, raising=False)
    lib = he.load_library()
    he.reset_overrides(lib)
    yield lib
    he.reset_overrides(lib)


def wanted(lib):
    w = ctypes.c_int32(-7)
    assert lib.nss_csr_value_codes_wanted(1000, ctypes.byref(w)) == 0
    return w.value


class Recorder:
    """stands in for a library: the setters of the table, less `missing`, record their calls"""

    def __init__(self, missing=()):
        self.calls = []
        for o in he.OVERRIDES.values():
            if o.setter not in missing:
                setattr(self, o.setter, functools.partial(self.record, o.setter))

    def record(self, setter, *args):
        self.calls.append((setter, args))
        return 0


def test_the_table_names_every_setter(lib):
    ints = (ctypes.c_int32, ctypes.c_int64)
    setters = {name for name, (_, args) in he._signatures().items() if args and all(a in ints for a in args)}
    assert setters == {o.setter for o in he.OVERRIDES.values()} and len(setters) == len(he.OVERRIDES) == 14
    for name, o in he.OVERRIDES.items():
        assert len(o.default) == len(he._signatures()[o.setter][1]), name
        assert len(o.env) in (0, 1, len(o.default)), name         # none, the variable, or one per argument
        assert he._in_force[name] == o.default, name
    assert he.OVERRIDES["cond_fuse"].default == (0,) and he.OVERRIDES["amg_batch"].default == (1,)
    assert he.OVERRIDES["dispatch"].default == (-2, 0, 0)


def test_round_trip(lib):
    assert wanted(lib) == 0
    with he.overrides(lib, value_codes=1):
        assert wanted(lib) == 1 and he._in_force["value_codes"] == (1,)
    assert wanted(lib) == 0 and he._in_force["value_codes"] == (-1,)
    with pytest.raises(ZeroDivisionError):
        with he.overrides(lib, value_codes=1):
            assert wanted(lib) == 1
            1 / 0
    assert wanted(lib) == 0 and he._in_force["value_codes"] == (-1,)


def test_blocks_nest(lib):
    with he.overrides(lib, value_codes=1, dispatch=(3, 0, 5)):
        with he.overrides(lib, value_codes=0, direct_rows=0):
            assert wanted(lib) == 0
            assert he._in_force["dispatch"] == (3, 0, 5) and he._in_force["direct_rows"] == (0,)
        assert wanted(lib) == 1 and he._in_force["direct_rows"] == (-1,)
    assert wanted(lib) == 0 and he._in_force == {name: o.default for name, o in he.OVERRIDES.items()}


def test_a_refused_value_raises_and_changes_nothing(lib):
    with pytest.raises(he.NssError, match="value_code_mode"):
        with he.overrides(lib, value_codes=7):
            raise AssertionError("the block must not run")
    assert wanted(lib) == 0 and he._in_force["value_codes"] == (-1,)
    with he.overrides(lib, value_codes=1):
        with pytest.raises(he.NssError):
            with he.overrides(lib, value_codes=0, block_codes=7):      # the first is set, then put back: to 1
                raise AssertionError("the block must not run")
        assert wanted(lib) == 1 and he._in_force["value_codes"] == (1,) and he._in_force["block_codes"] == (-1,)
    assert wanted(lib) == 0


def test_unknown_names_and_wrong_arity_raise_before_anything_is_set(lib):
    fake = Recorder()
    for bad in (dict(value_codes=1, no_such_switch=0), dict(value_codes=1, dispatch=3), dict(value_codes=(1, 2))):
        with pytest.raises((TypeError, KeyError)):
            with he.overrides(fake, **bad):
                raise AssertionError("the block must not run")
    assert fake.calls == [] and he._in_force["value_codes"] == (-1,)


def test_engine_method_is_the_same_call(lib):
    class Engine:
        overrides = he.HipEngine.overrides
    eng = Engine()
    eng.lib = lib
    with eng.overrides(value_codes=1):
        assert wanted(lib) == 1
    assert wanted(lib) == 0


def test_environment_sets_the_value_blocks_return_to(lib, monkeypatch):
    monkeypatch.setenv("NSS_VALUE_CODES", "1")
    fresh = he.load_library()
    assert wanted(fresh) == 1 and he._in_force["value_codes"] == (1,)
    with he.overrides(fresh, value_codes=0):
        assert wanted(fresh) == 0
    assert wanted(fresh) == 1                          # the value on entry, not the library default
    he.reset_overrides(fresh)
    assert wanted(fresh) == 0
    assert wanted(he.load_library()) == 1              # applied on every call


def test_environment_pass_over_the_table(lib, monkeypatch):
    fake = Recorder()
    he._apply_environment(fake)
    assert fake.calls == []                            # nothing set: nothing applied
    monkeypatch.setenv("NSS_FOLD_SUMS", "0")
    monkeypatch.setenv("NSS_DISPATCH_PLANES", "8")
    monkeypatch.setenv("NSS_DISPATCH_RUN", "5")
    monkeypatch.setenv("NSS_DISPATCH_MIN_PERIOD", "100")
    monkeypatch.setenv("NSS_AMG_BATCH", "")            # empty: as unset
    he._apply_environment(fake)
    assert sorted(fake.calls) == [("nss_bpcg1_fold_mode", (0,)), ("nss_bpcg2_fold_mode", (0,)),
                                  ("nss_csr_dispatch_mode", (8, 100, 5)), ("nss_minres_fold_mode", (0,))]
    assert he._in_force["dispatch"] == (8, 100, 5) and he._in_force["amg_batch"] == (1,)
    assert [he._in_force[k] for k in ("bpcg2_fold", "minres_fold", "bpcg1_fold", "lanczos_fold")] == [(0,)] * 3 + [(-1,)]
    monkeypatch.delenv("NSS_DISPATCH_RUN")
    monkeypatch.delenv("NSS_DISPATCH_MIN_PERIOD")      # the companions default to 0
    older = Recorder(missing=("nss_bpcg1_fold_mode",))
    he._apply_environment(older)                       # an entry point the library lacks is skipped
    assert sorted(older.calls) == [("nss_bpcg2_fold_mode", (0,)), ("nss_csr_dispatch_mode", (8, 0, 0)),
                                   ("nss_minres_fold_mode", (0,))]
    he.reset_overrides(older)
    assert ("nss_bpcg1_fold_mode", (-1,)) not in older.calls and ("nss_amg_batch_components", (1,)) in older.calls
    # the companions alone set nothing
    monkeypatch.delenv("NSS_DISPATCH_PLANES")
    monkeypatch.delenv("NSS_FOLD_SUMS")
    monkeypatch.setenv("NSS_DISPATCH_RUN", "5")
    fake = Recorder()
    he._apply_environment(fake)
    assert fake.calls == []
