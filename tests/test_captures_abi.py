"""Capturing groups on the CPU (needle_pattern_captures_info, needle_pattern_captures_tables, the argument checks of
needle_captures_spans_packed_dev; the Python surface of Pattern around them): the tagged automaton that the capture kernel walks is
exported and walked here (captures_cases.walk) against the reference's own expectations (tests/golden/captures.txt: JDK results) and
against re.fullmatch, on hand-written patterns and on a seeded fuzz; the refusals carry their reason."""
import ctypes
import inspect
import re
import time

import numpy as np
import pytest

from captures_cases import (CASE_INSENSITIVE, MUST_REFUSE, MUST_WORK, dictionary_regex, fuzz_patterns, fuzz_texts, re_groups, read_fixture, to_re,
                            walk)

VP, U64, I = ctypes.c_void_p, ctypes.c_uint64, ctypes.c_int


@pytest.fixture(scope="module")
def lib():
    from needle_amd import build
    build.build()
    from needle_amd import _lib
    return _lib.lib()


def compile_(regex, flags=0):
    from needle_amd.pattern import DFACompiler
    return DFACompiler.compile(regex, "c", flags)


def test_symbols_and_signatures(lib):
    from needle_amd import _lib
    from needle_amd.pattern import Pattern
    for n in ("needle_pattern_captures_info", "needle_pattern_captures_tables", "needle_captures_spans_packed_dev"):
        assert n in _lib.EXPORTS and hasattr(lib, n), n
    P = ctypes.POINTER
    assert lib.needle_captures_spans_packed_dev.argtypes == [VP, P(_lib.PackedView), VP, VP, VP, VP, VP, U64, VP]
    assert lib.needle_pattern_captures_info.argtypes == [VP, I, P(_lib.CapturesInfo)]
    assert _lib.CAPTURES_MAX_GROUPS == 16
    sig = lambda f: list(inspect.signature(f).parameters)
    assert sig(Pattern.captures_info) == ["self", "char_width"] and sig(Pattern.group_count) == ["self"]
    assert sig(Pattern.captures_spans_packed) == ["self", "data", "offsets", "span_offsets", "start", "end", "stream", "out"]
    assert sig(Pattern.find_all_groups_packed)[:3] == ["self", "data", "offsets"]
    assert sig(Pattern.extract_group_packed)[:4] == ["self", "data", "offsets", "g"]
    assert sig(Pattern.find_all_groups_strings) == ["self", "strings"] and sig(Pattern.find_all_groups_bytes) == ["self", "rows"]
    assert sig(Pattern.find_all_groups_utf8_packed)[:3] == ["self", "data", "offsets"]


def test_fixture(lib):
    """The reference's captures.txt: 4 rows with `$` do not compile here, the 3 nullable loops are refused, the other 19 give the
    fixture's strings on the fixture's [start, end) -- and re.fullmatch's positions."""
    from needle_amd.pattern import PatternSyntaxException
    rows = read_fixture()
    assert len(rows) == 26
    n_dollar = n_loop = n_ok = 0
    for pat, hay, start, end, want in rows:
        if "$" in pat:
            with pytest.raises(PatternSyntaxException):
                compile_(pat)
            n_dollar += 1
            continue
        p = compile_(pat)
        info = p.captures_info()
        assert info["n_groups"] == len(want) == p.group_count(), pat
        if pat in ("(A*|B)*", "(A*|B)+", "(A*|B)*A"):
            assert not info["available"] and info["reason"] == "NULLABLE_LOOP", pat
            n_loop += 1
            continue
        assert info["available"] and info["reason"] is None, (pat, info)
        t = hay[start:end]
        got = walk(p.captures_tables(), t)
        assert got is not None and got[0] == (0, len(t)), (pat, hay)
        assert [None if s < 0 else t[s:e] for s, e in got[1:]] == want, (pat, hay, got)
        assert got == re_groups(re.compile(pat), t), (pat, hay)
        n_ok += 1
    assert (n_dollar, n_loop, n_ok) == (4, 3, 19)


@pytest.mark.parametrize("case", range(len(MUST_WORK)))
def test_must_work(lib, case):
    regex, flags, cw, texts = MUST_WORK[case]
    p = compile_(regex, flags)
    info = p.captures_info(cw)
    assert info["available"] and info["reason"] is None, info
    cre = re.compile(to_re(regex), re.IGNORECASE if flags & CASE_INSENSITIVE else 0)
    assert info["n_groups"] == cre.groups == p.group_count()
    assert info["n_slots"] == info["max_threads"] * 2 * info["n_groups"] and info["lds_bytes"] % 16 == 0
    t = p.captures_tables(cw)
    some = False
    for text in texts:
        want = re_groups(cre, text)
        assert walk(t, text) == want, (regex, text)
        some = some or want is not None
    assert some and not all(re_groups(cre, x) for x in texts), "texts: matching and non-matching ones"


def test_loop_keeps_earlier_span(lib):
    assert walk(compile_("(a(b)?)+").captures_tables(), "aba") == [(0, 3), (2, 3), (1, 2)]


@pytest.mark.parametrize("regex,reason", MUST_REFUSE)
def test_refused(lib, regex, reason):
    from needle_amd import _lib
    p = compile_(regex)
    info = p.captures_info()
    assert not info["available"] and info["reason"] == reason
    assert info["n_groups"] == re.compile(regex).groups
    assert lib.needle_pattern_captures_tables(p._h, 1, None, None, None, 0, None, 0, None, 0, None, 0) == _lib.ERR_UNSUPPORTED
    assert reason in _lib.last_error()


def test_no_regex(lib):
    from needle_amd.pattern import Pattern, PatternException
    p = compile_("(a)(b)")
    assert p.captures_info()["available"]
    t = p.tables()
    for q in (Pattern.from_bytes(p.to_bytes()), Pattern.from_tables(t["class_map"], t["stride"], t["dfas"], t.get("fixed_len", -1))):
        info = q.captures_info()
        assert not info["available"] and info["reason"] == "NO_REGEX" and info["n_groups"] == -1
        with pytest.raises(PatternException):
            q.group_count()


def test_too_big_stops_at_the_budget(lib):
    p = compile_(dictionary_regex())
    t0 = time.time()
    info = p.captures_info()
    assert time.time() - t0 < 5.0
    assert not info["available"] and info["reason"] == "TOO_BIG" and info["n_groups"] == 1


def test_fuzz(lib):
    """2000 seeded patterns x 100 texts against re.fullmatch; at most 1 % refused, and then only as TOO_BIG."""
    pats = fuzz_patterns()
    assert len(pats) == 2000
    refused = matched = 0
    for i, regex in enumerate(pats):
        p = compile_(regex)
        info = p.captures_info()
        if not info["available"]:
            assert info["reason"] == "TOO_BIG", (regex, info)
            refused += 1
            continue
        t, cre = p.captures_tables(), re.compile(regex)
        for text in fuzz_texts(i):
            want = re_groups(cre, text)
            assert walk(t, text) == want, (regex, text)
            matched += want is not None
    print("fuzz: %d of %d patterns refused (TOO_BIG), %d matching texts" % (refused, len(pats), matched))
    assert refused <= len(pats) // 100 and matched > 10000


def test_argument_checks_need_no_device(lib):
    from needle_amd import _lib
    p = compile_("([0-9]+)-([0-9]+)")
    data = np.frombuffer(b"1-2 33-4", dtype=np.uint8).copy()
    offsets = np.array([0, 3, 8], dtype=np.uint64)
    span_off = np.array([0, 1, 2], dtype=np.uint64)
    start, end = np.array([0, 1], dtype=np.int32), np.array([3, 5], dtype=np.int32)
    gs, ge = np.zeros((3, 2), np.int32), np.zeros((3, 2), np.int32)

    def view(data_ptr=data.ctypes.data, cw=1, n=2, off=offsets.ctypes.data):
        v = _lib.PackedView()
        v.data, v.char_width, v.n_rows, v.offsets = data_ptr, cw, n, off
        return v
    fn = lib.needle_captures_spans_packed_dev
    so, st, en, a, b = span_off.ctypes.data, start.ctypes.data, end.ctypes.data, gs.ctypes.data, ge.ctypes.data
    bad = _lib.ERR_INVALID
    assert fn(None, ctypes.byref(view()), so, st, en, a, b, 2, None) == bad            # NULL pattern
    assert fn(p._h, None, so, st, en, a, b, 2, None) == bad                            # NULL view
    assert fn(p._h, ctypes.byref(view(off=None)), so, st, en, a, b, 2, None) == bad    # NULL offsets
    assert fn(p._h, ctypes.byref(view(cw=3)), so, st, en, a, b, 2, None) == bad        # bad char width
    assert fn(p._h, ctypes.byref(view(data_ptr=data.ctypes.data + 1)), so, st, en, a, b, 2, None) == bad
    assert fn(p._h, ctypes.byref(view()), None, st, en, a, b, 2, None) == bad          # NULL span offsets
    assert fn(p._h, ctypes.byref(view()), so, st, None, a, b, 2, None) == bad          # one of start / end
    assert fn(p._h, ctypes.byref(view()), so, st, en, None, b, 2, None) == bad         # a list, and no planes
    assert fn(p._h, ctypes.byref(view()), so, st, en, a, None, 2, None) == bad
    assert "planes" in _lib.last_error()
    assert fn(compile_("(a*)+")._h, ctypes.byref(view()), so, st, en, a, b, 2, None) == _lib.ERR_UNSUPPORTED
    assert "NULLABLE_LOOP" in _lib.last_error()
    assert fn(p._h, ctypes.byref(view(n=0)), so, None, None, None, None, 0, None) == _lib.NEEDLE_OK  # no rows: nothing to do
    info = _lib.CapturesInfo()
    assert lib.needle_pattern_captures_info(None, 1, ctypes.byref(info)) == bad
    assert lib.needle_pattern_captures_info(p._h, 1, None) == bad
    assert lib.needle_pattern_captures_info(p._h, 3, ctypes.byref(info)) == bad
    assert lib.needle_pattern_captures_tables(p._h, 0, None, None, None, 0, None, 0, None, 0, None, 0) == bad
    small = np.zeros(1, np.int32)
    assert lib.needle_pattern_captures_tables(p._h, 1, None, small.ctypes.data, None, 1, None, 0, None, 0, None, 0) == bad
