"""CPU-side checks of the packed device entries (needle_matches_packed_dev / needle_contained_in_packed_dev /
needle_find_packed_dev): exported, every argument check answers NEEDLE_ERR_INVALID before any device call, and an empty
batch returns NEEDLE_OK without touching a device -- none of this needs a GPU."""
import ctypes

import numpy as np
import pytest

NAMES = ("needle_matches_packed_dev", "needle_contained_in_packed_dev", "needle_find_packed_dev")


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
_bm = np.zeros(1, dtype=np.uint64)
_st = np.zeros(2, dtype=np.int32)
_en = np.zeros(2, dtype=np.int32)


def _view(data_ptr=None, cw=1, n=2, offsets_ptr=None):
    from needle_amd import _lib
    v = _lib.PackedView()
    v.data = _data.ctypes.data if data_ptr is None else data_ptr
    v.char_width, v.n_rows = cw, n
    v.offsets = _offsets.ctypes.data if offsets_ptr is None else offsets_ptr
    return v


def _call(lib, name, h, v, bm=True, st=True, en=True):
    bmp = _bm.ctypes.data if bm else None
    vp = ctypes.byref(v) if v is not None else None
    if name == "needle_find_packed_dev":
        return getattr(lib, name)(h, vp, bmp, _st.ctypes.data if st else None, _en.ctypes.data if en else None, None)
    return getattr(lib, name)(h, vp, bmp, None)


@pytest.mark.parametrize("name", NAMES)
def test_validation_without_device(lib, pattern, name):
    from needle_amd import _lib
    h = pattern._h
    bad = [
        (None, _view(), {}),                              # NULL pattern
        (h, None, {}),                                    # NULL view
        (h, _view(offsets_ptr=0), {}),                    # NULL offsets
        (h, _view(), {"bm": False}),                      # NULL bitmap
        (h, _view(cw=0), {}),                             # char_width not 1 | 2
        (h, _view(cw=3), {}),
        (h, _view(cw=4), {}),
        (h, _view(data_ptr=_data.ctypes.data + 1), {}),   # data not 4-byte aligned
        (h, _view(data_ptr=_data.ctypes.data + 2, cw=2), {}),
    ]
    if name == "needle_find_packed_dev":
        bad += [(h, _view(), {"st": False}), (h, _view(), {"en": False})]
    for ph, v, kw in bad:
        assert _call(lib, name, ph, v, **kw) == _lib.ERR_INVALID, (name, kw)
        assert lib.needle_last_error()


@pytest.mark.parametrize("name", NAMES)
def test_empty_batch_is_ok(lib, pattern, name):
    from needle_amd import _lib
    for cw in (1, 2):
        assert _call(lib, name, pattern._h, _view(cw=cw, n=0)) == _lib.NEEDLE_OK


def test_python_numpy_inputs_keep_the_host_path(pattern):
    """Pattern.*_packed take the host path for numpy inputs (the device path is for device tensors only): the keywords exist and
    a numpy call still dispatches to the host entries -- here stopped by their own validation before any device is used."""
    import inspect
    from needle_amd.pattern import Pattern
    for m in ("matches_packed", "contained_in_packed", "find_packed"):
        params = inspect.signature(getattr(Pattern, m)).parameters
        assert "stream" in params and "out" in params, m
