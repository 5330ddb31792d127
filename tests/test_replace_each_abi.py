"""CPU-side checks of the replace-each entries (needle_replace_each_lengths_packed_dev / needle_replace_each_fill_packed_dev /
needle_set_replace_each_packed_host): exported with the documented signatures, every argument check answers NEEDLE_ERR_INVALID with a
message before any device call (also for an empty batch), an empty batch returns NEEDLE_OK without touching a device, the Python
surface and its ValueErrors -- none of this needs a GPU.  And `splice_each`, the ten-line reference every GPU test of the feature
compares against, pinned to hand-written answers."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

from test_replace_abi import splice

NAMES = ("needle_replace_each_lengths_packed_dev", "needle_replace_each_fill_packed_dev", "needle_set_replace_each_packed_host")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def splice_each(row, matches, choices, repls):
    """row[0:s_0] + X_0 + row[e_0:s_1] + ... + X_last + row[e_last:], X_j = repls[c_j] when 0 <= c_j < len(repls), else the match's own
    text row[s_j:e_j] -- the definition of "replace each" (include/needle_hip.h).  str, list and numpy rows alike; numpy in, numpy out."""
    parts, pos = [], 0
    for (s, e), c in zip(matches, choices):
        parts.append(row[pos:s])
        parts.append(repls[int(c)] if 0 <= int(c) < len(repls) else row[s:e])
        pos = e
    parts.append(row[pos:])
    if isinstance(row, np.ndarray):
        return np.concatenate([np.asarray(x, dtype=row.dtype) for x in parts])
    out = parts[0]
    for x in parts[1:]:
        out = out + x
    return out


def test_reference_splice_each():
    assert splice_each("abc123def45", [(3, 6), (9, 11)], [0, 1], ["#", "<n>"]) == "abc#def<n>"
    assert splice_each("abc123def45", [(3, 6), (9, 11)], [-1, 0], ["#", "<n>"]) == "abc123def#"
    assert splice_each("abc123def45", [(3, 6), (9, 11)], [2, 0], ["#", "<n>"]) == "abc123def#"       # a choice behind the table: kept
    assert splice_each("aabbcc", [(0, 2), (2, 4), (4, 6)], [1, -1, 0], ["-", ""]) == "bb-"           # deleted, kept, replaced
    assert splice_each("dab", [(0, 0)], [-1], ["XY"]) == "dab"                                         # a kept empty match
    assert splice_each("dab", [(0, 0)], [0], ["XY"]) == "XYdab"
    assert splice_each("abc", [(1, 2)], [-2 ** 31], ["#"]) == "abc" and splice_each("abc", [(1, 2)], [2 ** 31 - 1], ["#"]) == "abc"
    for row, matches in (("abc123def45", [(3, 6), (9, 11)]), ("aabbcc", [(0, 2), (2, 4), (4, 6)]), ("", []), ("x", [(0, 1)]), ("ab", [(0, 1), (1, 1)])):
        for repl in ("", "#", "<number>"):
            assert splice_each(row, matches, [0] * len(matches), [repl]) == splice(row, matches, repl)
    got = splice_each(np.array([1, 2, 3, 4, 5], np.uint16), [(1, 3), (3, 4)], [1, 7], [np.zeros(0, np.uint16), np.array([9, 9, 9], np.uint16)])
    assert got.dtype == np.uint16 and got.tolist() == [1, 9, 9, 9, 4, 5]


@pytest.fixture(scope="module")
def lib():
    from needle_amd import build
    build.build()
    from needle_amd import _lib
    return _lib.lib()


@pytest.fixture(scope="module")
def pattern(lib):
    from needle_amd.pattern import DFACompiler
    return DFACompiler.compile("[0-9]+|[a-c]+")


@pytest.fixture(scope="module")
def pset(lib):
    from needle_amd.pattern import DFACompiler, PatternSet
    return PatternSet([DFACompiler.compile("[0-9]+"), DFACompiler.compile("[a-c]+")])


def test_symbols_exported_with_the_documented_signatures(lib):
    from needle_amd import _lib
    header = open(os.path.join(ROOT, "include", "needle_hip.h")).read()
    squeeze = lambda s: re.sub(r"\s+", " ", s)
    flat = squeeze(header)
    for n in NAMES:
        assert hasattr(lib, n), n
        assert n in _lib.EXPORTS, n
    assert "#define NEEDLE_REPLACE_MAX_CHOICES 256" in header and _lib.REPLACE_MAX_CHOICES == 256
    assert "#define NEEDLE_CHOICE_INDEX 0" in header and _lib.CHOICE_INDEX == 0
    assert "#define NEEDLE_CHOICE_LOWEST_BIT 1" in header and _lib.CHOICE_LOWEST_BIT == 1
    assert squeeze("int needle_replace_each_lengths_packed_dev(const needle_packed_view *rows, const uint64_t *d_match_offsets, "
                   "const int32_t *d_start, const int32_t *d_end, const void *d_choice, int choice_form, const uint32_t *repl_offsets, "
                   "uint32_t n_repl, uint64_t *d_out_lengths, void *hip_stream);") in flat
    assert squeeze("int needle_replace_each_fill_packed_dev(const needle_packed_view *rows, const uint64_t *d_match_offsets, "
                   "const int32_t *d_start, const int32_t *d_end, const void *d_choice, int choice_form, const void *repl, "
                   "const uint32_t *repl_offsets, uint32_t n_repl, const uint64_t *d_out_offsets, void *d_out_data, void *hip_stream);") in flat
    assert squeeze("int needle_set_replace_each_packed_host(const needle_pattern_set *s, const needle_pattern *p, "
                   "const needle_packed_view *rows, const void *repl, const uint32_t *repl_offsets, uint32_t n_repl, uint64_t *out_offsets, "
                   "void *out_data, uint64_t capacity, uint64_t *total);") in flat
    assert len(lib.needle_replace_each_lengths_packed_dev.argtypes) == 10
    assert len(lib.needle_replace_each_fill_packed_dev.argtypes) == 12
    assert len(lib.needle_set_replace_each_packed_host.argtypes) == 10


# host buffers stand in for device pointers: the calls must refuse before any of them is dereferenced or a device is used
_data = np.zeros(64, dtype=np.uint8)
_offsets = np.array([0, 3, 7], dtype=np.uint64)
_moff = np.zeros(3, dtype=np.uint64)
_st = np.zeros(2, dtype=np.int32)
_en = np.zeros(2, dtype=np.int32)
_ch = np.zeros(2, dtype=np.int32)
_lens = np.zeros(2, dtype=np.uint64)
_ooff = np.zeros(3, dtype=np.uint64)
_out = np.zeros(64, dtype=np.uint8)
_repl = np.zeros(8192, dtype=np.uint8)
_total = ctypes.c_uint64(0)
_ROFF = np.array([0, 1, 4], dtype=np.uint32)  # two entries: 1 and 3 units


def _view(data_ptr=None, cw=1, n=2, offsets_ptr=None):
    from needle_amd import _lib
    v = _lib.PackedView()
    v.data = _data.ctypes.data if data_ptr is None else data_ptr
    v.char_width, v.n_rows = cw, n
    v.offsets = _offsets.ctypes.data if offsets_ptr is None else offsets_ptr
    return v


def _table(roff):
    """(pointer or None, n_repl) of a replacement-offsets array; None stands for a NULL pointer with n_repl 2."""
    if roff is None:
        return None, 2
    roff = np.ascontiguousarray(roff, dtype=np.uint32)
    return roff, roff.size - 1


def _lengths(lib, v, moff=True, roff=_ROFF, n_repl=None, form=0, out=True):
    keep, n = _table(roff)
    return lib.needle_replace_each_lengths_packed_dev(ctypes.byref(v) if v is not None else None, _moff.ctypes.data if moff else None, _st.ctypes.data,
                                                      _en.ctypes.data, _ch.ctypes.data, form, keep.ctypes.data if keep is not None else None,
                                                      n if n_repl is None else n_repl, _lens.ctypes.data if out else None, None)


def _fill(lib, v, moff=True, repl=True, roff=_ROFF, n_repl=None, form=0, ooff=True, out=True, out_ptr=None):
    keep, n = _table(roff)
    outp = (_out.ctypes.data if out_ptr is None else out_ptr) if out else None
    return lib.needle_replace_each_fill_packed_dev(ctypes.byref(v) if v is not None else None, _moff.ctypes.data if moff else None, _st.ctypes.data,
                                                   _en.ctypes.data, _ch.ctypes.data, form, _repl.ctypes.data if repl else None,
                                                   keep.ctypes.data if keep is not None else None, n if n_repl is None else n_repl,
                                                   _ooff.ctypes.data if ooff else None, outp, None)


def _host(lib, s, h, v, repl=True, roff=_ROFF, n_repl=None, ooff=True, out=True, capacity=64, total=True):
    keep, n = _table(roff)
    return lib.needle_set_replace_each_packed_host(s, h, ctypes.byref(v) if v is not None else None, _repl.ctypes.data if repl else None,
                                                   keep.ctypes.data if keep is not None else None, n if n_repl is None else n_repl,
                                                   _ooff.ctypes.data if ooff else None, _out.ctypes.data if out else None, capacity,
                                                   ctypes.byref(_total) if total else None)


def _refused(lib, rc, what):
    from needle_amd import _lib
    assert rc == _lib.ERR_INVALID, what
    assert lib.needle_last_error(), what


BAD_TABLES = [
    ("NULL offsets", dict(roff=None)),
    ("n_repl 0", dict(roff=np.zeros(258, np.uint32), n_repl=0)),
    ("n_repl 257", dict(roff=np.zeros(258, np.uint32), n_repl=257)),
    ("offsets[0] != 0", dict(roff=[1, 2, 3])),
    ("a decreasing pair", dict(roff=[0, 5, 4, 9])),
    ("a total above the limit", dict(roff=[0, 4000, 4097])),
    ("choice_form 2", dict(form=2)),
    ("choice_form -1", dict(form=-1)),
]


def test_validation_without_device(lib, pattern, pset):
    bad_views = [None, _view(offsets_ptr=0), _view(cw=0), _view(cw=3), _view(cw=4), _view(data_ptr=_data.ctypes.data + 1),
                 _view(data_ptr=_data.ctypes.data + 2, cw=2)]
    for i, v in enumerate(bad_views):
        _refused(lib, _lengths(lib, v), ("lengths, view", i))
        _refused(lib, _fill(lib, v), ("fill, view", i))
    for n in (2, 0):  # every refusal also with an empty batch: the arguments are checked first
        _refused(lib, _lengths(lib, _view(n=n), moff=False), ("lengths: NULL match offsets", n))
        _refused(lib, _lengths(lib, _view(n=n), out=False), ("lengths: NULL output", n))
        _refused(lib, _fill(lib, _view(n=n), moff=False), ("fill: NULL match offsets", n))
        _refused(lib, _fill(lib, _view(n=n), ooff=False), ("fill: NULL output offsets", n))
        _refused(lib, _fill(lib, _view(n=n), out=False), ("fill: NULL output", n))
        _refused(lib, _fill(lib, _view(n=n), out_ptr=_out.ctypes.data + 2), ("fill: output not 4-byte aligned", n))
        _refused(lib, _fill(lib, _view(n=n), repl=False), ("fill: NULL table with entries", n))
        for what, kw in BAD_TABLES:
            _refused(lib, _lengths(lib, _view(n=n), **kw), ("lengths", what, n))
            _refused(lib, _fill(lib, _view(n=n), **kw), ("fill", what, n))
    # the host entry
    s, h = pset._h, pattern._h
    _refused(lib, _host(lib, None, h, _view()), "host: NULL set")
    _refused(lib, _host(lib, s, None, _view()), "host: NULL pattern")
    for i, v in enumerate(bad_views[:5]):
        _refused(lib, _host(lib, s, h, v), ("host, view", i))
    for n in (2, 0):
        _refused(lib, _host(lib, s, h, _view(n=n), ooff=False), ("host: NULL out_offsets", n))
        _refused(lib, _host(lib, s, h, _view(n=n), total=False), ("host: NULL total", n))
        _refused(lib, _host(lib, s, h, _view(n=n), out=False, capacity=5), ("host: NULL text with capacity > 0", n))
        _refused(lib, _host(lib, s, h, _view(n=n), repl=False), ("host: NULL table with entries", n))
        _refused(lib, _host(lib, s, h, _view(n=n), roff=[0, 1, 2, 3]), ("host: three replacements for a set of two", n))
        _refused(lib, _host(lib, s, h, _view(n=n), roff=[0, 1]), ("host: one replacement for a set of two", n))
        for what, kw in BAD_TABLES[:6]:
            _refused(lib, _host(lib, s, h, _view(n=n), **kw), ("host", what, n))


def test_empty_batch_is_ok_and_the_limits(lib, pattern, pset):
    from needle_amd import _lib
    one_full = np.array([0, 4096], np.uint32)
    many = np.arange(257, dtype=np.uint32)           # 256 one-unit entries
    many_full = np.minimum(np.arange(257, dtype=np.uint32) * 17, 4096).astype(np.uint32)  # 256 entries, 4096 units
    for cw in (1, 2):
        for roff in (np.array([0, 0], np.uint32), np.array([0, 1], np.uint32), one_full, many, many_full):
            for form in (0, 1):
                assert _lengths(lib, _view(cw=cw, n=0), roff=roff, form=form) == _lib.NEEDLE_OK
                assert _fill(lib, _view(cw=cw, n=0), roff=roff, form=form) == _lib.NEEDLE_OK
        assert _fill(lib, _view(cw=cw, n=0), repl=False, roff=[0, 0, 0]) == _lib.NEEDLE_OK  # an empty table needs no units
        for roff in (np.array([0, 0, 0], np.uint32), np.array([0, 4096, 4096], np.uint32)):
            _ooff[0], _total.value = 7, 7
            assert _host(lib, pset._h, pattern._h, _view(cw=cw, n=0), roff=roff) == _lib.NEEDLE_OK
            assert _ooff[0] == 0 and _total.value == 0
        assert _host(lib, pset._h, pattern._h, _view(cw=cw, n=0), out=False, capacity=0) == _lib.NEEDLE_OK  # the sizing call


def test_python_surface(pset):
    from needle_amd.pattern import Pattern, PatternSet
    assert list(inspect.signature(Pattern.splice_each_packed).parameters) == [
        "data", "offsets", "match_offsets", "start", "end", "choice", "repls", "stream", "out", "out_start", "lowest_bit"]
    assert inspect.signature(Pattern.splice_each_packed).parameters["lowest_bit"].default is False
    assert list(inspect.signature(PatternSet.replace_each_packed).parameters) == ["self", "pattern", "data", "offsets", "repls", "stream", "out", "out_start"]
    assert list(inspect.signature(PatternSet.replace_each_strings).parameters) == ["self", "strings", "repls", "pattern"]
    assert list(inspect.signature(PatternSet.replace_each_bytes).parameters) == ["self", "rows", "repls", "pattern"]
    units, off = Pattern._repl_table(["", "#", "<n>", np.array([1, 255])], 1)
    assert units.dtype == np.uint8 and units.tolist() == [35, 60, 110, 62, 1, 255] and off.dtype == np.uint32 and off.tolist() == [0, 0, 1, 4, 6]
    units, off = Pattern._repl_table(["λ猫", ""], 2)
    assert units.dtype == np.uint16 and units.tolist() == [0x3BB, 0x732B] and off.tolist() == [0, 2, 2]
    assert Pattern._repl_table(["x"] * 256, 1)[1].tolist() == list(range(257))
    assert Pattern._repl_table(["", "x" * 4096, ""], 2)[1].tolist() == [0, 0, 4096, 4096]
    for bad in ([], ["x"] * 257, ["x" * 4097], ["x" * 2048, "y" * 2048, "z"], ["λ"]):
        with pytest.raises(ValueError):
            Pattern._repl_table(bad, 1)
    # one replacement per member, refused before anything is packed or sent
    with pytest.raises(ValueError):
        pset.replace_each_packed(None, np.zeros(4, np.uint8), np.array([0, 4], np.uint64), ["#"])
    with pytest.raises(ValueError):
        pset.replace_each_bytes([b"ab"], [b"#", b"<>", b"!"], pattern=object())
