"""CPU-side checks of the packed find-all entries (needle_count_matches_packed_dev / needle_find_all_csr_packed_dev /
needle_find_all_compact16_packed_dev / needle_find_all_csr_packed_host): exported, every argument check answers
NEEDLE_ERR_INVALID before any device call, and an empty batch returns NEEDLE_OK without touching a device -- none of this
needs a GPU."""
import ctypes

import numpy as np
import pytest

NAMES = ("needle_count_matches_packed_dev", "needle_find_all_csr_packed_dev", "needle_find_all_compact16_packed_dev",
         "needle_find_all_csr_packed_host")


@pytest.fixture(scope="module")
def lib():
    from needle_amd import build
    build.build()
    from needle_amd import _lib
    return _lib.lib()


@pytest.fixture(scope="module")
def pattern(lib):
    from needle_amd.pattern import DFACompiler
    return DFACompiler.compile("[0-9]+")


def test_symbols_exported(lib):
    from needle_amd import _lib
    for n in NAMES:
        assert hasattr(lib, n), n
        assert n in _lib.EXPORTS, n


# host buffers stand in for device pointers: the calls must refuse before any of them is dereferenced or a device is used
_data = np.zeros(64, dtype=np.uint8)
_offsets = np.array([0, 3, 7], dtype=np.uint64)
_u64 = np.zeros(8, dtype=np.uint64)
_i32 = np.zeros(8, dtype=np.int32)


def _view(data_ptr=None, cw=1, n=2, offsets_ptr=None):
    from needle_amd import _lib
    v = _lib.PackedView()
    v.data = _data.ctypes.data if data_ptr is None else data_ptr
    v.char_width, v.n_rows = cw, n
    v.offsets = _offsets.ctypes.data if offsets_ptr is None else offsets_ptr
    return v


def _call(lib, name, h, v, out=True, offs=True, st=True, en=True, total=True, max_per_row=32, cap=8):
    vp = ctypes.byref(v) if v is not None else None
    P = lambda a, keep: a.ctypes.data if keep else None
    fn = getattr(lib, name)
    if name == "needle_count_matches_packed_dev":
        return fn(h, vp, P(_i32, out), None)
    if name == "needle_find_all_csr_packed_dev":
        return fn(h, vp, P(_u64, offs), P(_i32, st), P(_i32, en), None, None)
    if name == "needle_find_all_compact16_packed_dev":
        return fn(h, vp, max_per_row, P(_u64, offs), P(_i32, out), cap, P(_u64, total), None, None)
    tot = ctypes.c_uint64(0)
    return fn(h, vp, P(_u64, offs), P(_i32, st), P(_i32, en), cap, ctypes.byref(tot) if total else None)


@pytest.mark.parametrize("name", NAMES)
def test_validation_without_device(lib, pattern, name):
    from needle_amd import _lib
    h = pattern._h
    bad = [
        (None, _view(), {}),                              # NULL pattern
        (h, None, {}),                                    # NULL view
        (h, _view(offsets_ptr=0), {}),                    # NULL offsets
        (h, _view(cw=0), {}),                             # char_width not 1 | 2
        (h, _view(cw=3), {}),
    ]
    if name != "needle_find_all_csr_packed_host":         # (host data needs no alignment)
        bad += [(h, _view(data_ptr=_data.ctypes.data + 1), {}), (h, _view(data_ptr=_data.ctypes.data + 2, cw=2), {})]
    if name == "needle_count_matches_packed_dev":
        bad += [(h, _view(), {"out": False})]
    elif name == "needle_find_all_csr_packed_dev":
        bad += [(h, _view(), {"offs": False}), (h, _view(), {"st": False}), (h, _view(), {"en": False})]
    elif name == "needle_find_all_compact16_packed_dev":
        bad += [(h, _view(), {"offs": False}), (h, _view(), {"out": False}), (h, _view(), {"total": False}),
                (h, _view(), {"max_per_row": 0}), (h, _view(), {"max_per_row": 4097})]
    else:
        bad += [(h, _view(), {"offs": False}), (h, _view(), {"st": False}), (h, _view(), {"en": False}), (h, _view(), {"total": False}),
                (h, _view(offsets_ptr=np.array([0, 5, 3], dtype=np.uint64).ctypes.data), {}),  # decreasing offsets
                (h, _view(data_ptr=0), {})]                                                    # NULL data with text
    for ph, v, kw in bad:
        assert _call(lib, name, ph, v, **kw) == _lib.ERR_INVALID, (name, kw)
        assert lib.needle_last_error()


@pytest.mark.parametrize("name", NAMES)
def test_empty_batch_is_ok(lib, pattern, name):
    from needle_amd import _lib
    for cw in (1, 2):
        assert _call(lib, name, pattern._h, _view(cw=cw, n=0)) == _lib.NEEDLE_OK


def test_python_entry_points():
    import inspect
    from needle_amd.pattern import Pattern
    for m, params in (("count_matches_packed", ("data", "offsets", "stream")), ("find_all_packed", ("data", "offsets", "stream")),
                      ("find_all_compact16_packed", ("data", "offsets", "max_per_row", "stream", "cap", "want_more")),
                      ("find_all_strings", ("strings",))):
        got = inspect.signature(getattr(Pattern, m)).parameters
        assert all(k in got for k in params), m


def test_route_predicate_matches_the_transducer_report():
    """Which patterns take the packed find-all kernel is what Pattern.find_all_transducer reports (one host predicate)."""
    from needle_amd.pattern import DFACompiler
    for rx, want in (("[0-9]+", 2), ("abc|de", 1), ("[a-z]{3}[a-z]*", 2), ("international|inter|nation", None), ("a*", None)):
        t = DFACompiler.compile(rx).find_all_transducer(1)
        assert (t["kind"] if t else None) == want, rx
