"""CPU-side checks of the UTF-8 entries (needle_utf16_lengths_from_utf8_packed_dev / needle_utf16_from_utf8_packed_dev /
needle_utf8_positions_packed_dev / needle_contained_in_utf8_packed_host / needle_find_all_csr_utf8_packed_host): exported with the
header's signatures, every argument check answers NEEDLE_ERR_INVALID with a message before any device call, an empty batch returns
NEEDLE_OK.  The rule restated in utf8_cases.py is pinned to CPython's decoder; the kernels' one statement of it (utf8_classify16) and
the host chunk layout run on the CPU as stand-alone programs under a sanitizer.  None of this needs a GPU."""
import ctypes
import os
import random
import re
import subprocess

import numpy as np
import pytest

import utf8_cases as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = ("needle_utf16_lengths_from_utf8_packed_dev", "needle_utf16_from_utf8_packed_dev", "needle_utf8_positions_packed_dev")
HOST = ("needle_contained_in_utf8_packed_host", "needle_find_all_csr_utf8_packed_host")


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
    flat = re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", "needle_hip.h")).read())
    for n in DEV + HOST + ("needle_utf8_window_bytes",):
        assert hasattr(lib, n), n
        assert n in _lib.EXPORTS, n
    assert "#define NEEDLE_UTF8_MAX_EXPANSION 1" in flat and _lib.UTF8_MAX_EXPANSION == 1
    for sig in ("int needle_utf16_lengths_from_utf8_packed_dev(const needle_packed_view *utf8, uint64_t *d_out_lengths, uint64_t *d_non_ascii, "
                "uint64_t *d_malformed, void *hip_stream);",
                "int needle_utf16_from_utf8_packed_dev(const needle_packed_view *utf8, const uint64_t *d_out_offsets, uint16_t *d_out_data, "
                "void *hip_stream);",
                "int needle_utf8_positions_packed_dev(const needle_packed_view *utf8, const uint64_t *d_list_offsets, const int32_t *d_unit_pos, "
                "int32_t *d_byte_pos, void *hip_stream);",
                "int needle_contained_in_utf8_packed_host(const needle_pattern *p, const needle_packed_view *utf8, uint64_t *bitmap, "
                "uint64_t *malformed);",
                "int needle_find_all_csr_utf8_packed_host(const needle_pattern *p, const needle_packed_view *utf8, uint64_t *offsets, "
                "int32_t *byte_start, int32_t *byte_end, uint64_t capacity, uint64_t *total, uint64_t *malformed);"):
        assert sig in flat, sig
    assert [len(getattr(lib, n).argtypes) for n in DEV + HOST] == [5, 4, 5, 4, 8]
    assert lib.needle_utf8_window_bytes() >= 64 and lib.needle_utf8_window_bytes() % 16 == 0


# host buffers stand in for device pointers: the calls must refuse before any of them is dereferenced or a device is used
_data = np.zeros(64, dtype=np.uint8)
_offsets = np.array([0, 3, 7], dtype=np.uint64)
_lens = np.zeros(2, dtype=np.uint64)
_words = np.zeros(1, dtype=np.uint64)
_uoff = np.zeros(3, dtype=np.uint64)
_units = np.zeros(64, dtype=np.uint16)
_loff = np.zeros(3, dtype=np.uint64)
_pos = np.zeros(4, dtype=np.int32)
_bpos = np.zeros(4, dtype=np.int32)
_total = ctypes.c_uint64(0)


def _view(data_ptr=None, cw=1, n=2, offsets_ptr=None):
    from needle_amd import _lib
    v = _lib.PackedView()
    v.data = _data.ctypes.data if data_ptr is None else data_ptr
    v.char_width, v.n_rows = cw, n
    v.offsets = _offsets.ctypes.data if offsets_ptr is None else offsets_ptr
    return v


def _ref(v):
    return ctypes.byref(v) if v is not None else None


def _lengths(lib, v, out=True):
    return lib.needle_utf16_lengths_from_utf8_packed_dev(_ref(v), _lens.ctypes.data if out else None, None, None, None)


def _fill(lib, v, uoff=True, out=True, out_ptr=None):
    return lib.needle_utf16_from_utf8_packed_dev(_ref(v), _uoff.ctypes.data if uoff else None,
                                                 (_units.ctypes.data if out_ptr is None else out_ptr) if out else None, None)


def _positions(lib, v, loff=True, pos=True, bpos=True):
    return lib.needle_utf8_positions_packed_dev(_ref(v), _loff.ctypes.data if loff else None, _pos.ctypes.data if pos else None,
                                                _bpos.ctypes.data if bpos else None, None)


def _contained(lib, h, v, bm=True):
    return lib.needle_contained_in_utf8_packed_host(h, _ref(v), _words.ctypes.data if bm else None, None)


def _find_all(lib, h, v, off=True, st=True, en=True, capacity=4, total=True):
    return lib.needle_find_all_csr_utf8_packed_host(h, _ref(v), _uoff.ctypes.data if off else None, _pos.ctypes.data if st else None,
                                                    _bpos.ctypes.data if en else None, capacity, ctypes.byref(_total) if total else None, None)


def _refused(lib, rc, what):
    from needle_amd import _lib
    assert rc == _lib.ERR_INVALID, what
    assert lib.needle_last_error(), what


def test_validation_without_device(lib, pattern):
    bad_views = [None, _view(offsets_ptr=0), _view(cw=0), _view(cw=2), _view(cw=3), _view(data_ptr=_data.ctypes.data + 1),
                 _view(data_ptr=_data.ctypes.data + 2)]
    for i, v in enumerate(bad_views):
        _refused(lib, _lengths(lib, v), ("lengths, view", i))
        _refused(lib, _fill(lib, v), ("fill, view", i))
        _refused(lib, _positions(lib, v), ("positions, view", i))
    _refused(lib, _lengths(lib, _view(), out=False), "lengths: NULL output")
    _refused(lib, _fill(lib, _view(), uoff=False), "fill: NULL output offsets")
    _refused(lib, _fill(lib, _view(), out=False), "fill: NULL output")
    _refused(lib, _fill(lib, _view(), out_ptr=_units.ctypes.data + 2), "fill: output not 4-byte aligned")
    _refused(lib, _positions(lib, _view(), loff=False), "positions: NULL list offsets")
    _refused(lib, _positions(lib, _view(), pos=False), "positions: NULL unit positions beside an output")
    _refused(lib, _positions(lib, _view(), bpos=False), "positions: NULL output beside unit positions")
    # ... also with an empty batch: the arguments are checked first
    _refused(lib, _lengths(lib, _view(n=0), out=False), "lengths, empty batch: NULL output")
    _refused(lib, _fill(lib, _view(n=0), out=False), "fill, empty batch: NULL output")
    _refused(lib, _fill(lib, _view(n=0, cw=2)), "fill, empty batch: char_width 2")
    _refused(lib, _positions(lib, _view(n=0), loff=False), "positions, empty batch: NULL list offsets")
    h = pattern._h
    _refused(lib, _contained(lib, None, _view()), "host containedIn: NULL pattern")
    _refused(lib, _find_all(lib, None, _view()), "host find-all: NULL pattern")
    for i, v in enumerate(bad_views[:5]):
        _refused(lib, _contained(lib, h, v), ("host containedIn, view", i))
        _refused(lib, _find_all(lib, h, v), ("host find-all, view", i))
    _refused(lib, _contained(lib, h, _view(), bm=False), "host containedIn: NULL bitmap")
    _refused(lib, _find_all(lib, h, _view(), off=False), "host find-all: NULL offsets")
    _refused(lib, _find_all(lib, h, _view(), total=False), "host find-all: NULL total")
    _refused(lib, _find_all(lib, h, _view(), st=False), "host find-all: NULL start with capacity > 0")
    _refused(lib, _find_all(lib, h, _view(), en=False), "host find-all: NULL end with capacity > 0")


def test_empty_batch_is_ok(lib, pattern):
    from needle_amd import _lib
    assert _lengths(lib, _view(n=0)) == _lib.NEEDLE_OK
    assert _fill(lib, _view(n=0)) == _lib.NEEDLE_OK
    assert _positions(lib, _view(n=0)) == _lib.NEEDLE_OK
    assert _positions(lib, _view(n=0), pos=False, bpos=False) == _lib.NEEDLE_OK  # an empty list: NULL arrays
    assert _contained(lib, pattern._h, _view(n=0)) == _lib.NEEDLE_OK
    _uoff[0], _total.value = 7, 7
    assert _find_all(lib, pattern._h, _view(n=0)) == _lib.NEEDLE_OK
    assert _uoff[0] == 0 and _total.value == 0
    assert _find_all(lib, pattern._h, _view(n=0), st=False, en=False, capacity=0) == _lib.NEEDLE_OK  # the sizing call


def test_python_surface():
    import inspect
    from needle_amd.pattern import Pattern, pack_bytes
    data, off = pack_bytes([b"ab", b"", "é".encode()])
    assert data.dtype == np.uint8 and data.tolist() == [97, 98, 0xC3, 0xA9] and off.dtype == np.uint64 and off.tolist() == [0, 2, 2, 4]
    assert pack_bytes([])[0].size == 0 and pack_bytes([])[1].tolist() == [0]
    assert list(inspect.signature(Pattern.utf16_from_utf8_packed).parameters)[:3] == ["data", "offsets", "stream"]
    assert list(inspect.signature(Pattern.utf8_positions_packed).parameters)[:5] == ["data", "offsets", "list_offsets", "unit_pos", "stream"]
    for m in ("contained_in_utf8_packed", "matches_utf8_packed", "find_all_utf8_packed"):
        assert list(inspect.signature(getattr(Pattern, m)).parameters)[:4] == ["self", "data", "offsets", "stream"], m
    assert list(inspect.signature(Pattern.find_all_bytes).parameters) == ["self", "rows"]
    assert list(inspect.signature(Pattern.replace_all_bytes).parameters) == ["self", "rows", "repl"]


# ---- the rule
@pytest.fixture(scope="module")
def rule_rows():
    rows = U.alphabet_rows() + U.random_rows(200000, seed=11)
    assert len(rows) == 406900 + 200000
    return rows


def test_the_rule_is_cpythons_decoder(rule_rows):
    for row in rule_rows:
        units, _ = U.utf8_units(row)
        assert np.array(units, "<u2").tobytes() == row.decode("utf-8", "replace").encode("utf-16-le", "surrogatepass"), row.hex()
        assert len(units) <= len(row)  # NEEDLE_UTF8_MAX_EXPANSION
    assert U.utf8_units(b"caf\xC3\xA9 \xF0\x9F\x98\x80!") == ([99, 97, 102, 0xE9, 32, 0xD83D, 0xDE00, 33], [0, 1, 2, 3, 5, 6, 10])
    assert U.utf8_units(b"\xE2\x82") == ([0xFFFD], [0]) and U.utf8_units(b"\xAC") == ([0xFFFD], [0])  # never a euro sign across rows
    assert U.utf8_units(b"\xEF\xBB\xBF\x00") == ([0xFEFF, 0], [0, 3])  # a BOM and a NUL are ordinary characters


def test_every_start_files_exactly_one_character(rule_rows):
    for row in rule_rows:
        units, starts = U.utf8_units(row)
        ends = starts[1:] + [len(row)]
        assert starts == sorted(set(starts)) and (not row or starts[0] == 0)
        n_units = 0
        for s, e in zip(starts, ends):
            ch = row[s:e].decode("utf-8", "replace")
            assert len(ch) == 1, (row.hex(), s, e)
            n_units += 2 if ord(ch) >= 0x10000 else 1
        assert n_units == len(units)
        b = U.unit_bytes(row)
        assert len(b) == len(units) + 1 and b == sorted(b) and b[-1] == len(row) and set(b[:-1]) == set(starts)
    row = b"a\xF0\x9F\x98\x80\xFFz"
    assert [U.byte_of_unit(row, p) for p in (-3, -1, 0, 1, 2, 3, 4, 5, 6, 99)] == [-1, -1, 0, 1, 1, 5, 6, 7, 7, 7]


# ---- the kernels' statement of the rule, and the host chunk layout, as stand-alone programs
def _compile(tmp_path_factory, name):
    exe = str(tmp_path_factory.mktemp(name) / name)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "c", name + ".cpp"), "-o", exe])
    return exe


def test_classify16_is_the_rule(tmp_path_factory):
    r = subprocess.run([_compile(tmp_path_factory, "utf8_classify_check")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.startswith("ok "), r.stderr[-2000:]


def test_host_chunk_layout(tmp_path_factory):
    exe = _compile(tmp_path_factory, "utf8_plan_check")
    rng = random.Random(5)
    cases = [(nr, text) for nr in (0, 1, 63, 64, 65, 4096) for text in (0, 1, 3, 4, 5, 1 << 20)]
    cases += [(rng.randrange(0, 1 << 22), rng.randrange(0, 1 << 32)) for _ in range(300)]
    r = subprocess.run([exe], input="".join("%d %d\n" % c for c in cases), capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = r.stdout.split("\n")[:-1]
    assert len(lines) == len(cases)
    for (nr, text), ln in zip(cases, lines):
        *at, total = [int(x) for x in ln.split()]
        words = (nr + 63) // 64 * 8
        sizes = [max(text, 4), (nr + 1) * 8, nr * 8, (nr + 1) * 8, words, words, words, nr * 4, (nr + 1) * 8, max(2 * text, 4)]
        end = 0
        for o, b in zip(at, sizes):  # in order, 16-byte aligned, no overlap
            assert o % 16 == 0 and o >= end
            end = o + b
        assert total >= end and total >= text + 2 * text + sum(sizes[1:9])  # the chunk, its UTF-16 form and the lists fit what is reserved
        assert sizes[9] >= 2 * text
