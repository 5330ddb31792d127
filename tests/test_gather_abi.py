"""CPU-side checks of the gather entries (needle_gather_spans_lengths_packed_dev / needle_gather_spans_fill_packed_dev /
needle_split_spans_packed_dev / needle_gather_chunk_spans / needle_gather_matches_packed_host): exported with the documented signatures,
every argument check answers NEEDLE_ERR_INVALID with a message before any device call, an empty batch returns NEEDLE_OK without touching
a device -- none of this needs a GPU.  And gather_ref / split_list_ref (tests/gather_cases.py), the references every GPU test of the
feature compares against, pinned to hand-written answers and, through the oracle's match lists, to CPython's re.findall / re.split."""
import ctypes
import os
import re

import numpy as np
import pytest

from gather_cases import gather_ref, split_list_ref

NAMES = ("needle_gather_spans_lengths_packed_dev", "needle_gather_spans_fill_packed_dev", "needle_split_spans_packed_dev",
         "needle_gather_chunk_spans", "needle_gather_matches_packed_host")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def extract(row, spans):
    return gather_ref([row], [spans])[0]


def split(row, spans):
    return gather_ref([row], split_list_ref([row], [spans]))[0]


def test_references_by_hand():
    assert extract("abc123def45", [(3, 6), (9, 11)]) == ["123", "45"]
    assert split("abc123def45", [(3, 6), (9, 11)]) == ["abc", "def", ""]
    assert split_list_ref(["abc123def45"], [[(3, 6), (9, 11)]]) == [[(0, 3), (6, 9), (11, 11)]]
    assert extract("12ab", [(0, 2)]) == ["12"] and split("12ab", [(0, 2)]) == ["", "ab"]                       # a match at 0
    assert extract("aabbcc", [(0, 2), (2, 4), (4, 6)]) == ["aa", "bb", "cc"]                                   # touching matches
    assert split("aabbcc", [(0, 2), (2, 4), (4, 6)]) == ["", "", "", ""]
    assert extract("abc", [(0, 3)]) == ["abc"] and split("abc", [(0, 3)]) == ["", ""]                          # a whole-row match
    assert extract("", []) == [] and split("", []) == [""]                                                     # an empty row
    assert extract("", [(0, 0)]) == [""] and split("", [(0, 0)]) == ["", ""]
    assert extract("abc", []) == [] and split("abc", []) == ["abc"]                                            # no matches
    assert extract("dab", [(1, 1)]) == [""] and split("dab", [(1, 1)]) == ["d", "ab"]                          # an empty match
    row = "0123456789"                                                                                         # clamped spans
    assert extract(row, [(-3, 2)]) == ["01"] and extract(row, [(5, 99)]) == ["56789"] and extract(row, [(4, 1)]) == [""]
    assert extract(row, [(99, 120)]) == [""] and extract(row, [(-9, -2)]) == [""]
    assert split_list_ref([row], [[(-3, 2), (5, 99)]]) == [[(0, 0), (2, 5), (10, 10)]]
    assert split_list_ref([row], [[(4, 1)]]) == [[(0, 4), (4, 10)]]                                            # (4, 1) clamps to (4, 4)
    assert split_list_ref([row], [[(6, 8), (2, 4)]]) == [[(0, 6), (8, 8), (4, 10)]]                            # not monotone: end raised to start
    got = gather_ref([np.array([1, 2, 3, 4], np.uint16)], [[(1, 3), (1, 3), (0, 9)]])[0]                       # repeated, numpy rows
    assert [g.tolist() for g in got] == [[2, 3], [2, 3], [1, 2, 3, 4]] and got[0].dtype == np.uint16


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


# (regex, alphabet, whether two of its matches can touch)
RE_CASES = [("[0-9]+", "ab 0123456789", False), (", *", "ab, ,c ", True), ("ab|cd", "abcd ", True), ("abc+d|ab", "abcd", True)]


@pytest.mark.parametrize("regex,alphabet,touching", RE_CASES)
def test_references_against_re(lib, regex, alphabet, touching):
    """The oracle's find_all list through gather_ref is re.findall, through split_list_ref + gather_ref re.split: 3000 seeded rows of up
    to 40 chars per pattern.  Matches at 0, at the row's end and touching matches each occur hundreds of times."""
    from test_compile_matches_txt import oracle_for
    o, _ = oracle_for(regex, 0)
    rng = np.random.default_rng(len(regex))
    rows = ["".join(rng.choice(list(alphabet), int(k))) for k in rng.integers(0, 41, 3000)]
    lists = [o.find_all(r, limit=1 << 30) for r in rows]
    rx = re.compile(regex)
    assert sum(1 for l in lists if l and l[0][0] == 0) > 100 and sum(1 for r, l in zip(rows, lists) if l and l[-1][1] == len(r)) > 100
    assert not touching or sum(1 for l in lists for a, b in zip(l, l[1:]) if a[1] == b[0]) > 100
    assert gather_ref(rows, lists) == [rx.findall(r) for r in rows]
    assert gather_ref(rows, split_list_ref(rows, lists)) == [rx.split(r) for r in rows]


def test_symbols_exported_with_the_documented_signatures(lib):
    from needle_amd import _lib
    header = open(os.path.join(ROOT, "include", "needle_hip.h")).read()
    squeeze = lambda s: re.sub(r"\s+", " ", s)
    flat = squeeze(header)
    for n in NAMES:
        assert hasattr(lib, n), n
        assert n in _lib.EXPORTS, n
    assert "#define NEEDLE_GATHER_MATCHES 0" in header and "#define NEEDLE_GATHER_PIECES 1" in header
    assert (_lib.GATHER_MATCHES, _lib.GATHER_PIECES) == (0, 1)
    assert squeeze("int needle_gather_spans_lengths_packed_dev(const needle_packed_view *rows, const uint64_t *d_span_offsets, "
                   "const int32_t *d_start, const int32_t *d_end, uint64_t *d_out_lengths, void *hip_stream);") in flat
    assert squeeze("int needle_gather_spans_fill_packed_dev(const needle_packed_view *rows, const uint64_t *d_span_offsets, "
                   "const int32_t *d_start, const int32_t *d_end, const uint64_t *d_out_offsets, void *d_out_data, void *hip_stream);") in flat
    assert squeeze("int needle_split_spans_packed_dev(const needle_packed_view *rows, const uint64_t *d_match_offsets, const int32_t *d_start, "
                   "const int32_t *d_end, uint64_t *d_piece_offsets, int32_t *d_piece_start, int32_t *d_piece_end, void *hip_stream);") in flat
    assert "uint32_t needle_gather_chunk_spans(void);" in flat
    assert squeeze("int needle_gather_matches_packed_host(const needle_pattern *p, const needle_packed_view *rows, int mode, "
                   "uint64_t *span_offsets, uint64_t *out_offsets, uint64_t span_capacity, void *out_data, uint64_t unit_capacity, "
                   "uint64_t *total_spans, uint64_t *total_units);") in flat
    assert len(lib.needle_gather_spans_lengths_packed_dev.argtypes) == 6
    assert len(lib.needle_gather_spans_fill_packed_dev.argtypes) == 7
    assert len(lib.needle_split_spans_packed_dev.argtypes) == 8
    assert len(lib.needle_gather_matches_packed_host.argtypes) == 10
    assert lib.needle_gather_chunk_spans.restype is ctypes.c_uint32 and lib.needle_gather_chunk_spans() >= 64


# host buffers stand in for device pointers: the calls must refuse before any of them is dereferenced or a device is used
_data = np.zeros(64, dtype=np.uint8)
_offsets = np.array([0, 3, 7], dtype=np.uint64)
_soff = np.zeros(3, dtype=np.uint64)
_st = np.zeros(4, dtype=np.int32)
_en = np.zeros(4, dtype=np.int32)
_lens = np.zeros(4, dtype=np.uint64)
_ooff = np.zeros(5, dtype=np.uint64)
_out = np.zeros(64, dtype=np.uint8)
_poff = np.zeros(3, dtype=np.uint64)
_spans = ctypes.c_uint64(0)
_units = ctypes.c_uint64(0)


def _view(data_ptr=None, cw=1, n=2, offsets_ptr=None):
    from needle_amd import _lib
    v = _lib.PackedView()
    v.data = _data.ctypes.data if data_ptr is None else data_ptr
    v.char_width, v.n_rows = cw, n
    v.offsets = _offsets.ctypes.data if offsets_ptr is None else offsets_ptr
    return v


def _p(a, on=True):
    return a.ctypes.data if on else None


def _lengths(lib, v, soff=True, st=True, en=True, out=True):
    return lib.needle_gather_spans_lengths_packed_dev(ctypes.byref(v) if v is not None else None, _p(_soff, soff), _p(_st, st), _p(_en, en),
                                                      _p(_lens, out), None)


def _fill(lib, v, soff=True, st=True, en=True, ooff=True, out=True, out_ptr=None):
    outp = (_out.ctypes.data if out_ptr is None else out_ptr) if out else None
    return lib.needle_gather_spans_fill_packed_dev(ctypes.byref(v) if v is not None else None, _p(_soff, soff), _p(_st, st), _p(_en, en),
                                                   _p(_ooff, ooff), outp, None)


def _split(lib, v, soff=True, st=True, en=True, poff=True, ps=True, pe=True):
    return lib.needle_split_spans_packed_dev(ctypes.byref(v) if v is not None else None, _p(_soff, soff), _p(_st, st), _p(_en, en),
                                             _p(_poff, poff), _p(_st, ps), _p(_en, pe), None)


def _host(lib, h, v, mode=0, soff=True, ooff=True, span_cap=4, out=True, unit_cap=64, spans=True, units=True):
    return lib.needle_gather_matches_packed_host(h, ctypes.byref(v) if v is not None else None, mode, _p(_soff, soff), _p(_ooff, ooff), span_cap,
                                                 _p(_out, out), unit_cap, ctypes.byref(_spans) if spans else None,
                                                 ctypes.byref(_units) if units else None)


def _refused(lib, rc, what):
    from needle_amd import _lib
    assert rc == _lib.ERR_INVALID, what
    assert lib.needle_last_error(), what


def test_validation_without_device(lib, pattern):
    bad_views = [None, _view(offsets_ptr=0), _view(cw=0), _view(cw=3), _view(cw=4), _view(data_ptr=_data.ctypes.data + 1),
                 _view(data_ptr=_data.ctypes.data + 2), _view(data_ptr=_data.ctypes.data + 2, cw=2)]
    for n in (2, 0):  # (every one of them also with an empty batch: the arguments are checked first)
        for i, v in enumerate(bad_views):
            if v is not None:
                v.n_rows = n
            _refused(lib, _lengths(lib, v), ("lengths, view", i, n))
            _refused(lib, _fill(lib, v), ("fill, view", i, n))
            _refused(lib, _split(lib, v), ("split, view", i, n))
        _refused(lib, _lengths(lib, _view(n=n), soff=False), "lengths: NULL span offsets")
        _refused(lib, _lengths(lib, _view(n=n), out=False), "lengths: NULL output")
        _refused(lib, _lengths(lib, _view(n=n), st=False), "lengths: NULL start alone")
        _refused(lib, _lengths(lib, _view(n=n), en=False), "lengths: NULL end alone")
        _refused(lib, _fill(lib, _view(n=n), soff=False), "fill: NULL span offsets")
        _refused(lib, _fill(lib, _view(n=n), ooff=False), "fill: NULL output offsets")
        _refused(lib, _fill(lib, _view(n=n), out=False), "fill: NULL output")
        _refused(lib, _fill(lib, _view(n=n), out_ptr=_out.ctypes.data + 1), "fill: output misaligned by 1")
        _refused(lib, _fill(lib, _view(n=n), out_ptr=_out.ctypes.data + 2), "fill: output misaligned by 2")
        _refused(lib, _fill(lib, _view(n=n, cw=2), out_ptr=_out.ctypes.data + 2), "fill: 16-bit output misaligned by 2")
        _refused(lib, _fill(lib, _view(n=n), st=False), "fill: NULL start alone")
        _refused(lib, _fill(lib, _view(n=n), en=False), "fill: NULL end alone")
        _refused(lib, _split(lib, _view(n=n), soff=False), "split: NULL match offsets")
        _refused(lib, _split(lib, _view(n=n), poff=False), "split: NULL piece offsets")
        _refused(lib, _split(lib, _view(n=n), ps=False), "split: NULL piece start")
        _refused(lib, _split(lib, _view(n=n), pe=False), "split: NULL piece end")
        _refused(lib, _split(lib, _view(n=n), st=False), "split: NULL start alone")
        _refused(lib, _split(lib, _view(n=n), en=False), "split: NULL end alone")
    # the host entry
    h = pattern._h
    _refused(lib, _host(lib, None, _view()), "host: NULL pattern")
    for i, v in enumerate(bad_views[:5]):
        _refused(lib, _host(lib, h, v), ("host, view", i))
    for n in (2, 0):
        for mode in (-1, 2, 7):
            _refused(lib, _host(lib, h, _view(n=n), mode=mode), ("host: mode", mode))
        _refused(lib, _host(lib, h, _view(n=n), soff=False), "host: NULL span_offsets")
        _refused(lib, _host(lib, h, _view(n=n), spans=False), "host: NULL total_spans")
        _refused(lib, _host(lib, h, _view(n=n), units=False), "host: NULL total_units")
        _refused(lib, _host(lib, h, _view(n=n), ooff=False, span_cap=3), "host: NULL out_offsets with capacity > 0")
        _refused(lib, _host(lib, h, _view(n=n), out=False, unit_cap=5), "host: NULL text with capacity > 0")


def test_empty_batch_and_null_lists_are_ok(lib, pattern):
    from needle_amd import _lib
    for cw in (1, 2):
        assert _lengths(lib, _view(cw=cw, n=0)) == _lib.NEEDLE_OK
        assert _fill(lib, _view(cw=cw, n=0)) == _lib.NEEDLE_OK
        assert _split(lib, _view(cw=cw, n=0)) == _lib.NEEDLE_OK
        # start and end both NULL: the caller's word that the list is empty -- nothing to gather, no device is touched
        assert _lengths(lib, _view(cw=cw, n=0), st=False, en=False) == _lib.NEEDLE_OK
        assert _fill(lib, _view(cw=cw, n=0), st=False, en=False) == _lib.NEEDLE_OK
        assert _split(lib, _view(cw=cw, n=0), st=False, en=False) == _lib.NEEDLE_OK
        assert _lengths(lib, _view(cw=cw), st=False, en=False) == _lib.NEEDLE_OK
        assert _fill(lib, _view(cw=cw), st=False, en=False) == _lib.NEEDLE_OK
        for mode in (0, 1):
            _soff[0], _ooff[0], _spans.value, _units.value = 7, 7, 7, 7
            assert _host(lib, pattern._h, _view(cw=cw, n=0), mode=mode) == _lib.NEEDLE_OK
            assert _soff[0] == 0 and _ooff[0] == 0 and _spans.value == 0 and _units.value == 0
            assert _host(lib, pattern._h, _view(cw=cw, n=0), mode=mode, ooff=False, span_cap=0, out=False, unit_cap=0) == _lib.NEEDLE_OK  # sizing
    assert (_lens == 0).all() and (_out == 0).all() and (_poff == 0).all()


def test_python_surface():
    import inspect
    from needle_amd.pattern import Pattern
    sig = lambda f: list(inspect.signature(f).parameters)
    assert sig(Pattern.gather_spans_packed) == ["data", "offsets", "span_offsets", "start", "end", "stream", "out", "out_start"]
    assert sig(Pattern.split_spans_packed)[:5] == ["data", "offsets", "match_offsets", "start", "end"]
    assert sig(Pattern.select_rows_packed)[:3] == ["data", "offsets", "bits"]
    for m in ("extract_all_packed", "split_packed", "grep_packed"):
        assert sig(getattr(Pattern, m))[:3] == ["self", "data", "offsets"], m
    for m in ("extract_all_strings", "split_strings", "grep_strings"):
        assert sig(getattr(Pattern, m)) == ["self", "strings"], m
    for m in ("extract_all_bytes", "split_bytes"):
        assert sig(getattr(Pattern, m)) == ["self", "rows"], m
    for m in ("gather_spans_packed", "split_spans_packed", "select_rows_packed"):
        assert isinstance(inspect.getattr_static(Pattern, m), staticmethod), m
