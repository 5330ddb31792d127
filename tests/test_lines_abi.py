"""CPU-side checks of the line splitter's entries (needle_lines_tile_units / needle_lines_tiles / needle_lines_count_packed_dev /
needle_lines_fill_packed_dev): exported with the documented signatures, every argument check answers NEEDLE_ERR_INVALID with a message
before any device call, an empty batch returns NEEDLE_OK without touching a device -- none of this needs a GPU.  And lines_ref
(tests/lines_cases.py), the reference every GPU test of the feature compares against, pinned by hand, exhaustively against
bytes.splitlines, on the 16-bit look-alikes of the terminators, and against decoding ill-formed UTF-8 before or after the split."""
import ctypes
import itertools
import os
import random
import re

import numpy as np
import pytest

from lines_cases import batch_ref, lines_ref, tile_counts_ref

NAMES = ("needle_lines_tile_units", "needle_lines_tiles", "needle_lines_count_packed_dev", "needle_lines_fill_packed_dev")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def split(b, keep=False):
    return [bytes(l) for l in lines_ref(b, keep)]


def test_reference_by_hand():
    assert split(b"") == [] and split(b"", True) == []
    assert split(b"\n") == [b""] and split(b"\n", True) == [b"\n"]
    assert split(b"a\n") == [b"a"] and split(b"a") == [b"a"] and split(b"a\n", True) == [b"a\n"]
    assert split(b"\r\r\n") == [b"", b""] and split(b"\r\r\n", True) == [b"\r", b"\r\n"]
    assert split(b"a\r\nb\rc\nd") == [b"a", b"b", b"c", b"d"]
    assert split(b"a\r\nb\rc\nd", True) == [b"a\r\n", b"b\r", b"c\n", b"d"]
    assert split(b"\n\r") == [b"", b""] and split(b"\n\r", True) == [b"\n", b"\r"]
    # the lookahead never leaves the document: '\r' at the end of one, '\n' at the start of the next are two terminators
    text, off, doc = batch_ref([b"a\r", b"\nb"], True, np.uint8)
    assert bytes(text) == b"a\r\nb" and off.tolist() == [0, 2, 3, 4] and doc.tolist() == [0, 1, 3]
    text, off, doc = batch_ref([b"a\r", b"\nb"], False, np.uint8)
    assert bytes(text) == b"ab" and off.tolist() == [0, 1, 1, 2] and doc.tolist() == [0, 1, 3]
    text, off, doc = batch_ref([b"", b"x\ny", b"", b""], False, np.uint8)
    assert bytes(text) == b"xy" and off.tolist() == [0, 1, 2] and doc.tolist() == [0, 0, 2, 2, 2]
    ev, kept = tile_counts_ref([b"ab\ncd\r\n", b"e"], 3, 4, 4)  # units 3 .. 11 of the data, tiles of 4
    assert ev.tolist() == [0, 1, 2, 0] and kept.tolist() == [1, 3, 1, 0]


def test_reference_against_splitlines_exhaustively():
    """All 9841 strings over {a, \\n, \\r} of up to 8 units, both modes; lines = events, kept units = non-terminator units."""
    count = 0
    for k in range(9):
        for t in itertools.product(b"a\n\r", repeat=k):
            b = bytes(t)
            assert split(b) == b.splitlines() and split(b, True) == b.splitlines(keepends=True), b
            assert sum(len(l) for l in split(b)) == b.count(b"a") and b"".join(split(b, True)) == b
            count += 1
    assert count == 9841


def test_reference_on_the_16_bit_look_alikes():
    """Terminators are compared as whole code units: 0x0A0A, 0x010A, 0x0D00, 0x2028, 0x0085 do not split (Java's rule)."""
    alike = [0x0A0A, 0x010A, 0x0D00, 0x2028, 0x0085, 0x0A00, 0x0D0D]
    doc = [0x61] + alike + [0x62]
    assert lines_ref(doc, False) == [doc] and lines_ref(doc, True) == [doc]
    for x in alike:
        assert lines_ref([0x0D, x, 0x0A, x], True) == [[0x0D], [x, 0x0A], [x]]
        assert lines_ref([0x0D, x, 0x0A, x], False) == [[], [x], [x]]
    text, off, _ = batch_ref([np.array([0x2028, 0x0A, 0x0085], np.uint16)], False, np.uint16)
    assert text.dtype == np.uint16 and text.tolist() == [0x2028, 0x0085] and off.tolist() == [0, 1, 2]


def test_split_and_decode_commute_on_ill_formed_utf8():
    """0x0A and 0x0D never occur inside a multi-byte sequence, and a sequence cut short by a terminator is one maximal subpart either way:
    splitting the bytes then decoding each line equals decoding the file then splitting the text.  20 000 seeded strings."""
    rng = random.Random(8)
    atoms = [b"a", b"\n", b"\r", b"\r\n", b"\xc3", b"\xa9", b"\xe4", b"\xb8", b"\xad", b"\xf0", b"\x9f", b"\x98", b"\x80", b"\xff", b"\xed",
             b"\xa0", b"\xc0", b"\xe0", b"\xf4", b"\x90", "é".encode(), "中".encode(), "😀".encode()]
    differ = 0
    for _ in range(20000):
        b = b"".join(rng.choice(atoms) for _ in range(rng.randint(0, 12)))
        before = [bytes(l).decode("utf-8", "replace") for l in lines_ref(b, False)]
        after = ["".join(map(chr, l)) for l in lines_ref([ord(c) for c in b.decode("utf-8", "replace")], False)]
        assert before == after, b
        differ += b.decode("utf-8", "replace") != b.decode("latin-1")
    assert differ > 10000


@pytest.fixture(scope="module")
def lib():
    from needle_amd import build
    build.build()
    from needle_amd import _lib
    return _lib.lib()


def test_symbols_exported_with_the_documented_signatures(lib):
    from needle_amd import _lib
    header = open(os.path.join(ROOT, "include", "needle_hip.h")).read()
    squeeze = lambda s: re.sub(r"\s+", " ", s)
    flat = squeeze(header)
    for n in NAMES:
        assert hasattr(lib, n), n
        assert n in _lib.EXPORTS, n
    assert "#define NEEDLE_LINES_KEEP_ENDS 1u" in header and _lib.LINES_KEEP_ENDS == 1
    assert "uint32_t needle_lines_tile_units(uint32_t char_width);" in flat
    assert "uint64_t needle_lines_tiles(uint64_t data_units, uint32_t char_width);" in flat
    assert squeeze("int needle_lines_count_packed_dev(const needle_packed_view *docs, uint64_t data_units, uint32_t flags, "
                   "uint64_t *d_tile_lines, uint64_t *d_tile_units, void *hip_stream);") in flat
    assert squeeze("int needle_lines_fill_packed_dev(const needle_packed_view *docs, uint64_t data_units, uint32_t flags, "
                   "const uint64_t *d_tile_line_base, const uint64_t *d_tile_unit_base, uint64_t *d_out_offsets, void *d_out_data, "
                   "uint64_t *d_doc_line_offsets, void *hip_stream);") in flat
    assert len(lib.needle_lines_count_packed_dev.argtypes) == 6 and len(lib.needle_lines_fill_packed_dev.argtypes) == 9
    assert lib.needle_lines_tile_units.restype is ctypes.c_uint32 and lib.needle_lines_tiles.restype is ctypes.c_uint64


def test_tile_arithmetic(lib):
    t1, t2 = lib.needle_lines_tile_units(1), lib.needle_lines_tile_units(2)
    assert t1 >= 256 and t1 == 2 * t2 and t1 % 16 == 0
    for cw in (0, 3, 4, 8):
        assert lib.needle_lines_tile_units(cw) == 0 and lib.needle_lines_tiles(100, cw) == 0
    for cw, T in ((1, t1), (2, t2)):
        for units, want in ((0, 0), (1, 1), (T - 1, 1), (T, 1), (T + 1, 2), (3 * T + 5, 4), (T << 33, 1 << 33), ((T << 33) + 1, (1 << 33) + 1)):
            assert lib.needle_lines_tiles(units, cw) == want, (cw, units)


# host buffers stand in for device pointers: the calls must refuse before any of them is dereferenced or a device is used
_data = np.zeros(64, dtype=np.uint8)
_offsets = np.array([0, 3, 7], dtype=np.uint64)
_tl = np.zeros(4, dtype=np.uint64)
_tu = np.zeros(4, dtype=np.uint64)
_lb = np.zeros(5, dtype=np.uint64)
_ub = np.zeros(5, dtype=np.uint64)
_oo = np.zeros(9, dtype=np.uint64)
_out = np.zeros(64, dtype=np.uint8)
_dl = np.zeros(3, dtype=np.uint64)


def _view(data_ptr=None, cw=1, n=2, offsets_ptr=None):
    from needle_amd import _lib
    v = _lib.PackedView()
    v.data = _data.ctypes.data if data_ptr is None else data_ptr
    v.char_width, v.n_rows = cw, n
    v.offsets = _offsets.ctypes.data if offsets_ptr is None else offsets_ptr
    return v


def _p(a, on=True):
    return a.ctypes.data if on else None


def _count(lib, v, units=64, flags=0, tl=True, tu=True):
    return lib.needle_lines_count_packed_dev(ctypes.byref(v) if v is not None else None, units, flags, _p(_tl, tl), _p(_tu, tu), None)


def _fill(lib, v, units=64, flags=0, lb=True, ub=True, oo=True, out=True, out_ptr=None, dl=True):
    outp = (_out.ctypes.data if out_ptr is None else out_ptr) if out else None
    return lib.needle_lines_fill_packed_dev(ctypes.byref(v) if v is not None else None, units, flags, _p(_lb, lb), _p(_ub, ub), _p(_oo, oo), outp,
                                            _p(_dl, dl), None)


def _refused(lib, rc, what):
    from needle_amd import _lib
    assert rc == _lib.ERR_INVALID, what
    assert lib.needle_last_error(), what


def test_validation_without_device(lib):
    bad_views = [None, _view(offsets_ptr=0), _view(cw=0), _view(cw=3), _view(cw=4), _view(data_ptr=_data.ctypes.data + 1),
                 _view(data_ptr=_data.ctypes.data + 2), _view(data_ptr=_data.ctypes.data + 2, cw=2)]
    for n, units in ((2, 64), (0, 64), (2, 0)):  # (every one of them also with an empty batch: the arguments are checked first)
        for i, v in enumerate(bad_views):
            if v is not None:
                v.n_rows = n
            for flags in (0, 1):
                _refused(lib, _count(lib, v, units, flags), ("count, view", i, n, flags))
                _refused(lib, _fill(lib, v, units, flags), ("fill, view", i, n, flags))
        for flags in (2, 3, 4, 0x80000000, 0xFFFFFFFE):
            _refused(lib, _count(lib, _view(n=n), units, flags), ("count: flags", flags))
            _refused(lib, _fill(lib, _view(n=n), units, flags), ("fill: flags", flags))
        for flags in (0, 1):
            _refused(lib, _count(lib, _view(n=n), units, flags, tl=False), "count: NULL tile lines")
            _refused(lib, _fill(lib, _view(n=n), units, flags, lb=False), "fill: NULL line base")
            _refused(lib, _fill(lib, _view(n=n), units, flags, oo=False), "fill: NULL output offsets")
        _refused(lib, _count(lib, _view(n=n), units, 0, tu=False), "count: NULL tile units, STRIP")
        _refused(lib, _fill(lib, _view(n=n), units, 0, ub=False), "fill: NULL unit base, STRIP")
        _refused(lib, _fill(lib, _view(n=n), units, 0, out=False), "fill: NULL text, STRIP")
        _refused(lib, _fill(lib, _view(n=n), units, 0, out_ptr=_out.ctypes.data + 1), "fill: text misaligned by 1")
        _refused(lib, _fill(lib, _view(n=n), units, 0, out_ptr=_out.ctypes.data + 2), "fill: text misaligned by 2")
        _refused(lib, _fill(lib, _view(n=n, cw=2), units, 0, out_ptr=_out.ctypes.data + 2), "fill: 16-bit text misaligned by 2")


def test_empty_batch_is_ok_and_writes_nothing(lib):
    from needle_amd import _lib
    for a in (_tl, _tu, _oo, _dl):
        a[:] = 77
    _out[:] = 77
    for cw in (1, 2):
        for n, units in ((0, 64), (2, 0), (0, 0)):
            for flags in (0, 1):
                assert _count(lib, _view(cw=cw, n=n), units, flags) == _lib.NEEDLE_OK
                assert _fill(lib, _view(cw=cw, n=n), units, flags) == _lib.NEEDLE_OK
                assert _fill(lib, _view(cw=cw, n=n), units, flags, dl=False) == _lib.NEEDLE_OK
            # what KEEP_ENDS does not need may be NULL
            assert _count(lib, _view(cw=cw, n=n), units, 1, tu=False) == _lib.NEEDLE_OK
            assert _fill(lib, _view(cw=cw, n=n), units, 1, ub=False, out=False) == _lib.NEEDLE_OK
            assert _fill(lib, _view(cw=cw, n=n), units, 1, out_ptr=_out.ctypes.data + 1) == _lib.NEEDLE_OK  # (ignored under KEEP_ENDS)
    assert all((a == 77).all() for a in (_tl, _tu, _oo, _dl, _out))


def test_python_surface():
    import inspect
    from needle_amd import pattern
    sig = lambda f: list(inspect.signature(f).parameters)
    assert sig(pattern.lines_packed) == ["data", "offsets", "keep_ends", "stream", "out", "out_start", "line_start"]
    assert sig(pattern.lines_of_bytes) == ["buf", "keep_ends"]
    assert sig(pattern.Pattern.grep_lines_bytes) == ["self", "buf"] and sig(pattern.Pattern.count_lines_bytes) == ["self", "buf"]
    d = inspect.signature(pattern.lines_packed).parameters
    assert d["offsets"].default is None and d["keep_ends"].default is False and d["out_start"].default == 0 and d["line_start"].default == 0
