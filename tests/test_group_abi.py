"""CPU-side checks of needle_group_spans_packed_dev / needle_group_spans_work_bytes: exported with the documented signatures, every
argument check answers NEEDLE_ERR_INVALID with a message before any device call, the workspace query and the layout header
(needle_amd/csrc/needle_group.h, through tests/c/group_plan_check.cpp built with -fsanitize=address,undefined) -- none of this needs a
GPU.  And group_ref / distinct_ref (tests/group_cases.py), the model every GPU test of the feature compares against, pinned by hand."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from group_cases import NONE, distinct_ref, group_ref
from set_spans_cases import spans_from_lists

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_model_by_hand():
    """A dozen spans over three rows: repeats across rows, a clamped span that equals a plain one, empty spans from three sources, an
    absent span, a text with a unit 0 against its prefix; the first two entries of the list are nobody's."""
    rows = ["abcab", "", "ab\0"]
    per_row = [[(0, 2), (3, 5), (2, 3), (9, 12), (4, 1), (-3, 2), (-1, -1)], [(0, 0), (0, 5)], [(0, 2), (0, 3), (0, 99), (-2, -7)]]
    spans = spans_from_lists(per_row, lead=2)
    first, count = group_ref(rows, spans, fill_first=7, fill_count=9)
    #        lead  ab ab c  "" "" ab abs "" ""  ab  ab\0 ab\0 abs
    assert first.tolist() == [7, 7, 2, 2, 4, 5, 5, 2, NONE, 5, 5, 2, 12, 12, NONE]
    assert count.tolist() == [9, 9, 4, 4, 1, 4, 4, 4, 0, 4, 4, 4, 2, 2, 0]
    assert distinct_ref(rows, spans) == [("ab", 4), ("c", 1), ("", 4), ("ab\0", 2)]
    # numpy rows of 16-bit units: the same text in two rows, and a text that differs in its high byte only
    rows = [np.array([1, 2, 0x0101], np.uint16), np.array([0x0101, 1, 2, 1], np.uint16)]
    spans = spans_from_lists([[(0, 2), (2, 3)], [(1, 3), (0, 1), (3, 4)]])
    first, count = group_ref(rows, spans)
    assert first.tolist() == [0, 1, 0, 1, 4] and count.tolist() == [2, 2, 2, 2, 1]


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
    for n in ("needle_group_spans_work_bytes", "needle_group_spans_packed_dev"):
        assert hasattr(lib, n) and n in _lib.EXPORTS, n
    assert "#define NEEDLE_GROUP_NONE 0xFFFFFFFFFFFFFFFFull" in header and _lib.GROUP_NONE == NONE == 2 ** 64 - 1
    assert "uint64_t needle_group_spans_work_bytes(uint64_t max_spans);" in flat
    assert squeeze("int needle_group_spans_packed_dev(const needle_packed_view *rows, const uint64_t *d_span_offsets, const int32_t *d_start, "
                   "const int32_t *d_end, uint64_t max_spans, uint32_t hash_bits, void *d_work, uint64_t work_bytes, uint64_t *d_first, "
                   "uint32_t *d_count, uint32_t *d_status, void *hip_stream);") in flat
    assert lib.needle_group_spans_work_bytes.restype is ctypes.c_uint64 and lib.needle_group_spans_work_bytes.argtypes == [ctypes.c_uint64]
    at = lib.needle_group_spans_packed_dev.argtypes
    assert len(at) == 12 and at[4] is ctypes.c_uint64 and at[5] is ctypes.c_uint32 and at[7] is ctypes.c_uint64
    # the header says what hash_bits is for, and what is out of scope
    block = header[header.index("Distinct spans and their counts"):header.index("#define NEEDLE_GROUP_NONE")]
    assert "hash_bits" in block and "tests reach the comparison path" in block and "Out of scope: a chunked _host entry" in block


def test_python_surface():
    import inspect
    from needle_amd.pattern import Pattern
    sig = lambda f: list(inspect.signature(f).parameters)
    assert sig(Pattern.group_spans_packed) == ["data", "offsets", "span_offsets", "start", "end", "stream", "hash_bits"]
    assert inspect.signature(Pattern.group_spans_packed).parameters["hash_bits"].default == 64
    assert sig(Pattern.distinct_spans_packed)[:5] == ["data", "offsets", "span_offsets", "start", "end"]
    assert sig(Pattern.distinct_matches_packed)[:3] == ["self", "data", "offsets"]
    assert sig(Pattern.distinct_rows_packed)[:2] == ["data", "offsets"]
    assert sig(Pattern.count_distinct_strings) == ["self", "strings"] and sig(Pattern.count_distinct_bytes) == ["self", "rows"]
    assert sig(Pattern.count_distinct_group_strings) == ["self", "strings", "g"]
    for m in ("group_spans_packed", "distinct_spans_packed", "distinct_rows_packed"):
        assert isinstance(inspect.getattr_static(Pattern, m), staticmethod), m


# host buffers stand in for device pointers: the calls must refuse before any of them is dereferenced or a device is used
_data = np.zeros(64, dtype=np.uint8)
_offsets = np.array([0, 3, 7], dtype=np.uint64)
_soff = np.zeros(3, dtype=np.uint64)
_st = np.zeros(4, dtype=np.int32)
_en = np.zeros(4, dtype=np.int32)
_first = np.full(4, 5, dtype=np.uint64)
_count = np.full(4, 5, dtype=np.uint32)
_status = np.full(1, 5, dtype=np.uint32)
_work = np.zeros(1 << 14, dtype=np.uint64)  # (numpy aligns large buffers to 16 bytes; asserted below)


def _view(data_ptr=None, cw=1, n=2, offsets_ptr=None):
    from needle_amd import _lib
    v = _lib.PackedView()
    v.data = _data.ctypes.data if data_ptr is None else data_ptr
    v.char_width, v.n_rows = cw, n
    v.offsets = _offsets.ctypes.data if offsets_ptr is None else offsets_ptr
    return v


def _p(a, on=True):
    return a.ctypes.data if on else None


def _group(lib, v, soff=True, st=True, en=True, max_spans=4, hash_bits=64, work=True, work_ptr=None, work_bytes=None, first=True, count=True,
           status=True):
    wb = int(lib.needle_group_spans_work_bytes(min(max_spans, 4))) if work_bytes is None else work_bytes
    wp = (_work.ctypes.data if work_ptr is None else work_ptr) if work else None
    return lib.needle_group_spans_packed_dev(ctypes.byref(v) if v is not None else None, _p(_soff, soff), _p(_st, st), _p(_en, en), max_spans,
                                             hash_bits, wp, wb, _p(_first, first), _p(_count, count), _p(_status, status), None)


def _refused(lib, rc, what):
    from needle_amd import _lib
    assert rc == _lib.ERR_INVALID, what
    assert lib.needle_last_error(), what


def test_validation_without_device(lib):
    assert _work.ctypes.data % 16 == 0 and _work.nbytes >= lib.needle_group_spans_work_bytes(4)
    bad_views = [None, _view(offsets_ptr=0), _view(cw=0), _view(cw=3), _view(cw=4), _view(data_ptr=_data.ctypes.data + 1),
                 _view(data_ptr=_data.ctypes.data + 2), _view(data_ptr=_data.ctypes.data + 2, cw=2)]
    for n in (2, 0):  # (every one of them also with an empty batch: the arguments are checked first)
        for i, v in enumerate(bad_views):
            if v is not None:
                v.n_rows = n
            _refused(lib, _group(lib, v), ("view", i, n))
        _refused(lib, _group(lib, _view(n=n), soff=False), "NULL span offsets")
        _refused(lib, _group(lib, _view(n=n), st=False), "NULL start alone")
        _refused(lib, _group(lib, _view(n=n), en=False), "NULL end alone")
        _refused(lib, _group(lib, _view(n=n), st=False, en=False), "both lists NULL with max_spans > 0")
        _refused(lib, _group(lib, _view(n=n), first=False), "NULL first")
        _refused(lib, _group(lib, _view(n=n), count=False), "NULL count")
        _refused(lib, _group(lib, _view(n=n), status=False), "NULL status")
        _refused(lib, _group(lib, _view(n=n), work=False), "NULL workspace")
        _refused(lib, _group(lib, _view(n=n), work_ptr=_work.ctypes.data + 8), "workspace misaligned")
        _refused(lib, _group(lib, _view(n=n), work_bytes=int(lib.needle_group_spans_work_bytes(4)) - 1), "workspace one byte short")
        _refused(lib, _group(lib, _view(n=n), work_bytes=0), "workspace of no bytes")
        _refused(lib, _group(lib, _view(n=n), st=False, en=False, max_spans=0, work_bytes=int(lib.needle_group_spans_work_bytes(0)) - 1),
                 "workspace one byte short for no spans")
        _refused(lib, _group(lib, _view(n=n), hash_bits=65), "hash_bits 65")
        _refused(lib, _group(lib, _view(n=n), hash_bits=2 ** 32 - 1), "hash_bits 2^32 - 1")
        _refused(lib, _group(lib, _view(n=n), max_spans=2 ** 32 - 1, work_bytes=2 ** 62), "max_spans above 2^32 - 2")
    assert (_first == 5).all() and (_count == 5).all() and (_status == 5).all() and not _work.any()


def slots_rule(max_spans):
    s = 64
    while s < 2 * max_spans:
        s *= 2
    return s


def test_work_bytes(lib):
    """Monotone, non-zero for 0, and never below the table of 2 * max_spans slots rounded up to a power of two (8 bytes a slot: word and
    count) plus the per-span arrays (8 + 8 + 8 + 4 bytes)."""
    q = lambda m: int(lib.needle_group_spans_work_bytes(m))
    sizes = [0, 1, 2, 31, 32, 33, 63, 64, 65, 1000, 4095, 4096, 4097, 10 ** 6, 46_600_000, 2 ** 31, 2 ** 32 - 2]
    got = [q(m) for m in sizes]
    assert got[0] >= 8 * 64 and all(a <= b for a, b in zip(got, got[1:]))
    for m, g in zip(sizes, got):
        need = 8 * slots_rule(m) + 28 * m
        assert need <= g <= need + 16 * 8 and g % 16 == 0, (m, g, need)
    for m in range(0, 300):
        assert q(m) <= q(m + 1)


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("group_plan") / "group_plan_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "c", "group_plan_check.cpp"), "-o", exe])

    def run(cases):
        text = "".join(" ".join(str(x) for x in c) + "\n" for c in cases)
        r = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr[-4000:]
        lines = r.stdout.split("\n")[:-1]
        assert len(lines) == len(cases)
        return [[int(x) for x in ln.split()] for ln in lines]
    return run


def test_layout_header_alone(plan, lib):
    """needle_group.h without HIP, under the sanitizers: the sections are 16-byte aligned, in order, disjoint and inside the total; the
    counts lie right behind the words, so that ONE range is cleared; the total is what the library's query answers."""
    sizes = [0, 1, 2, 3, 31, 32, 33, 64, 65, 127, 128, 129, 1000, 5000, 2 ** 20 + 1, 46_600_000, 2 ** 32 - 2]
    for m, (slots, addr, hsh, slot, ln, word, count, clear_at, clear_bytes, total) in zip(sizes, plan([("layout", m) for m in sizes])):
        assert slots == slots_rule(m) and slots & (slots - 1) == 0 and slots >= 2 * m
        sections = [(addr, 8 * m), (hsh, 8 * m), (slot, 8 * m), (ln, 4 * m), (word, 4 * slots), (count, 4 * slots)]
        at = 0
        for off, size in sections:
            assert off % 16 == 0 and off >= at, (m, sections)
            at = off + size
        assert at <= total and total % 16 == 0 and total > 0
        assert count == word + 4 * slots and (clear_at, clear_bytes) == (word, 8 * slots)
        assert total == lib.needle_group_spans_work_bytes(m)
    assert plan([("mask", b) for b in (0, 1, 8, 16, 63, 64)]) == [[0], [1], [255], [65535], [2 ** 63 - 1], [2 ** 64 - 1]]
    assert plan([("touch", m) for m in (0, 1, 2, 33, 1000, 100_000)]) == [[1]] * 6
