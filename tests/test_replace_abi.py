"""CPU-side checks of the replace entries (needle_replace_all_lengths_packed_dev / needle_replace_all_fill_packed_dev /
needle_replace_all_packed_host): exported with the documented signatures, every argument check answers NEEDLE_ERR_INVALID with a
message before any device call, an empty batch returns NEEDLE_OK without touching a device, the replacement's length limit -- none
of this needs a GPU.  And `splice`, the ten-line reference every GPU test of the feature compares against, pinned to hand-written
answers."""
import ctypes
import os
import re

import numpy as np
import pytest

NAMES = ("needle_replace_all_lengths_packed_dev", "needle_replace_all_fill_packed_dev", "needle_replace_all_packed_host")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def splice(row, matches, repl):
    """row[0:s_0] + repl + row[e_0:s_1] + repl + ... + repl + row[e_last:] for the match list [(s, e), ...] -- the definition of
    "replace all" (include/needle_hip.h).  Works on str, list and numpy rows alike; numpy in, numpy out."""
    parts, pos = [], 0
    for s, e in matches:
        parts.append(row[pos:s])
        parts.append(repl)
        pos = e
    parts.append(row[pos:])
    if isinstance(row, np.ndarray):
        return np.concatenate([np.asarray(x, dtype=row.dtype) for x in parts])
    out = parts[0]
    for x in parts[1:]:
        out = out + x
    return out


def test_reference_splice():
    assert splice("abc123def45", [(3, 6), (9, 11)], "#") == "abc#def#"
    assert splice("abc", [], "#") == "abc"
    assert splice("", [], "#") == ""
    assert splice("dab", [(0, 0)], "XY") == "XYdab"                  # an empty match at 0: pure insertion, then the row as it is
    assert splice("", [(0, 0)], "XY") == "XY"
    assert splice("aabbcc", [(0, 2), (2, 4), (4, 6)], "-") == "---"  # touching matches
    assert splice("aabbcc", [(0, 2), (2, 4), (4, 6)], "") == ""      # deletion of everything
    assert splice("xaybz", [(1, 2), (3, 4)], "") == "xyz"            # deletion
    assert splice("xaybz", [(1, 2), (3, 4)], "$1\\") == "x$1\\y$1\\z"  # the replacement is literal
    assert splice("ab", [(0, 1), (1, 1)], "Q") == "QQb"              # a match, then an empty one where it ended
    assert splice("x", [(0, 1)], "abc") == "abc"                     # first and last char at once
    got = splice(np.array([1, 2, 3, 4], np.uint16), [(1, 3)], np.array([9, 9, 9], np.uint16))
    assert got.dtype == np.uint16 and got.tolist() == [1, 9, 9, 9, 4]
    assert splice(np.array([1, 2], np.uint8), [(0, 2)], np.zeros(0, np.uint8)).size == 0


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


def test_symbols_exported_with_the_documented_signatures(lib):
    from needle_amd import _lib
    header = open(os.path.join(ROOT, "include", "needle_hip.h")).read()
    squeeze = lambda s: re.sub(r"\s+", " ", s)
    flat = squeeze(header)
    for n in NAMES:
        assert hasattr(lib, n), n
        assert n in _lib.EXPORTS, n
    assert "#define NEEDLE_REPLACE_MAX_UNITS 4096" in header and _lib.REPLACE_MAX_UNITS == 4096
    assert squeeze("int needle_replace_all_lengths_packed_dev(const needle_packed_view *rows, const uint64_t *d_match_offsets, "
                   "const int32_t *d_start, const int32_t *d_end, uint32_t repl_len, uint64_t *d_out_lengths, void *hip_stream);") in flat
    assert squeeze("int needle_replace_all_fill_packed_dev(const needle_packed_view *rows, const uint64_t *d_match_offsets, "
                   "const int32_t *d_start, const int32_t *d_end, const void *repl, uint32_t repl_len, const uint64_t *d_out_offsets, "
                   "void *d_out_data, void *hip_stream);") in flat
    assert squeeze("int needle_replace_all_packed_host(const needle_pattern *p, const needle_packed_view *rows, const void *repl, "
                   "uint32_t repl_len, uint64_t *out_offsets, void *out_data, uint64_t capacity, uint64_t *total);") in flat
    assert len(lib.needle_replace_all_lengths_packed_dev.argtypes) == 7
    assert len(lib.needle_replace_all_fill_packed_dev.argtypes) == 9
    assert len(lib.needle_replace_all_packed_host.argtypes) == 8


# host buffers stand in for device pointers: the calls must refuse before any of them is dereferenced or a device is used
_data = np.zeros(64, dtype=np.uint8)
_offsets = np.array([0, 3, 7], dtype=np.uint64)
_moff = np.zeros(3, dtype=np.uint64)
_st = np.zeros(2, dtype=np.int32)
_en = np.zeros(2, dtype=np.int32)
_lens = np.zeros(2, dtype=np.uint64)
_ooff = np.zeros(3, dtype=np.uint64)
_out = np.zeros(64, dtype=np.uint8)
_repl = np.zeros(8192, dtype=np.uint8)
_total = ctypes.c_uint64(0)


def _view(data_ptr=None, cw=1, n=2, offsets_ptr=None):
    from needle_amd import _lib
    v = _lib.PackedView()
    v.data = _data.ctypes.data if data_ptr is None else data_ptr
    v.char_width, v.n_rows = cw, n
    v.offsets = _offsets.ctypes.data if offsets_ptr is None else offsets_ptr
    return v


def _lengths(lib, v, moff=True, repl_len=1, out=True):
    return lib.needle_replace_all_lengths_packed_dev(ctypes.byref(v) if v is not None else None, _moff.ctypes.data if moff else None,
                                                     _st.ctypes.data, _en.ctypes.data, repl_len, _lens.ctypes.data if out else None, None)


def _fill(lib, v, moff=True, repl=True, repl_len=1, ooff=True, out=True, out_ptr=None):
    outp = (_out.ctypes.data if out_ptr is None else out_ptr) if out else None
    return lib.needle_replace_all_fill_packed_dev(ctypes.byref(v) if v is not None else None, _moff.ctypes.data if moff else None,
                                                  _st.ctypes.data, _en.ctypes.data, _repl.ctypes.data if repl else None, repl_len,
                                                  _ooff.ctypes.data if ooff else None, outp, None)


def _host(lib, h, v, repl=True, repl_len=1, ooff=True, out=True, capacity=64, total=True):
    return lib.needle_replace_all_packed_host(h, ctypes.byref(v) if v is not None else None, _repl.ctypes.data if repl else None, repl_len,
                                              _ooff.ctypes.data if ooff else None, _out.ctypes.data if out else None, capacity,
                                              ctypes.byref(_total) if total else None)


def _refused(lib, rc, what):
    from needle_amd import _lib
    assert rc == _lib.ERR_INVALID, what
    assert lib.needle_last_error(), what


def test_validation_without_device(lib, pattern):
    bad_views = [None, _view(offsets_ptr=0), _view(cw=0), _view(cw=3), _view(cw=4), _view(data_ptr=_data.ctypes.data + 1),
                 _view(data_ptr=_data.ctypes.data + 2, cw=2)]
    for i, v in enumerate(bad_views):
        _refused(lib, _lengths(lib, v), ("lengths, view", i))
        _refused(lib, _fill(lib, v), ("fill, view", i))
    _refused(lib, _lengths(lib, _view(), moff=False), "lengths: NULL match offsets")
    _refused(lib, _lengths(lib, _view(), out=False), "lengths: NULL output")
    _refused(lib, _lengths(lib, _view(), repl_len=4097), "lengths: replacement too long")
    _refused(lib, _fill(lib, _view(), moff=False), "fill: NULL match offsets")
    _refused(lib, _fill(lib, _view(), ooff=False), "fill: NULL output offsets")
    _refused(lib, _fill(lib, _view(), out=False), "fill: NULL output")
    _refused(lib, _fill(lib, _view(), out_ptr=_out.ctypes.data + 2), "fill: output not 4-byte aligned")
    _refused(lib, _fill(lib, _view(), repl=False, repl_len=1), "fill: NULL replacement of length 1")
    _refused(lib, _fill(lib, _view(), repl_len=4097), "fill: replacement too long")
    # every one of them also with an empty batch: the arguments are checked first
    _refused(lib, _lengths(lib, _view(n=0), repl_len=4097), "lengths, empty batch: replacement too long")
    _refused(lib, _fill(lib, _view(n=0), repl_len=4097), "fill, empty batch: replacement too long")
    _refused(lib, _fill(lib, _view(n=0), repl=False, repl_len=3), "fill, empty batch: NULL replacement")
    _refused(lib, _fill(lib, _view(n=0), out=False), "fill, empty batch: NULL output")
    # the host entry (the view's host-only checks: bad views, NULL outputs, the replacement)
    h = pattern._h
    _refused(lib, _host(lib, None, _view()), "host: NULL pattern")
    for i, v in enumerate(bad_views[:5]):
        _refused(lib, _host(lib, h, v), ("host, view", i))
    _refused(lib, _host(lib, h, _view(), ooff=False), "host: NULL out_offsets")
    _refused(lib, _host(lib, h, _view(), total=False), "host: NULL total")
    _refused(lib, _host(lib, h, _view(), out=False, capacity=5), "host: NULL text with capacity > 0")
    _refused(lib, _host(lib, h, _view(), repl=False, repl_len=2), "host: NULL replacement")
    _refused(lib, _host(lib, h, _view(), repl_len=4097), "host: replacement too long")


def test_empty_batch_is_ok_and_the_length_limit(lib, pattern):
    from needle_amd import _lib
    for cw in (1, 2):
        for repl_len in (0, 1, 4096):  # (4096 code units pass the validation, 4097 do not: above)
            assert _lengths(lib, _view(cw=cw, n=0), repl_len=repl_len) == _lib.NEEDLE_OK
            assert _fill(lib, _view(cw=cw, n=0), repl_len=repl_len) == _lib.NEEDLE_OK
            _ooff[0], _total.value = 7, 7
            assert _host(lib, pattern._h, _view(cw=cw, n=0), repl_len=repl_len) == _lib.NEEDLE_OK
            assert _ooff[0] == 0 and _total.value == 0
        assert _fill(lib, _view(cw=cw, n=0), repl=False, repl_len=0) == _lib.NEEDLE_OK  # deleting needs no replacement
        assert _host(lib, pattern._h, _view(cw=cw, n=0), out=False, capacity=0) == _lib.NEEDLE_OK  # the sizing call


def test_python_surface(pattern):
    import inspect
    from needle_amd.pattern import Pattern
    for m in ("replace_all_packed", "replace_first_packed"):
        assert list(inspect.signature(getattr(Pattern, m)).parameters)[:5] == ["self", "data", "offsets", "repl", "stream"], m
    assert list(inspect.signature(Pattern.splice_packed).parameters)[:7] == ["data", "offsets", "match_offsets", "start", "end", "repl", "stream"]
    assert list(inspect.signature(Pattern.replace_all_strings).parameters) == ["self", "strings", "repl"]
    # the replacement's encoding: literal code units of the rows' width
    assert Pattern._repl_units("a$1\\", 1).tolist() == [97, 36, 49, 92] and Pattern._repl_units("a", 1).dtype == np.uint8
    assert Pattern._repl_units("λ猫", 2).tolist() == [0x3BB, 0x732B] and Pattern._repl_units("", 2).size == 0
    assert Pattern._repl_units(np.array([1, 255]), 1).tolist() == [1, 255]
    with pytest.raises(ValueError):
        Pattern._repl_units("λ", 1)  # a char above 255 in 8-bit rows
    with pytest.raises(ValueError):
        Pattern._repl_units(np.array([256]), 1)
    with pytest.raises(ValueError):
        Pattern._repl_units("x" * 4097, 2)
    assert Pattern._repl_units("x" * 4096, 2).size == 4096
