"""needle_pattern_find_all_packed_filter / Pattern.find_all_packed_filter: whether the packed find-all entries
(needle_count_matches_packed_dev, needle_find_all_csr_packed_dev) take the n-gram filter kernel's find-all form for a pattern -- neither the
transducer nor the per-lane kernel takes it and the filter has a program for it: big dictionaries (the compressed automaton, hot rows /
the HBM table), on 8-bit rows, on UTF-16 rows of one page (Cyrillic) and of several (the WIDE filter).  needle_pattern_find_all_packed_route
keeps its answers for all of them.  Answered on the host: no GPU here."""
import ctypes
import functools

import pytest

ROUTES_ALL_CONVERSION = ["conversion"] * 4   # (char width 1, 2) x (count_only False, True)


@pytest.fixture(scope="module")
def lib():
    from needle_amd import build
    build.build()
    from needle_amd import _lib
    return _lib.lib()


@functools.lru_cache(maxsize=None)
def pattern(kind):
    from needle_amd import workload as W
    from needle_amd.pattern import DFACompiler
    latin = W.keywords(1000, min_len=6, max_len=8)
    cyr = lambda w: "".join(chr(0x0430 + ord(c) - 97) for c in w)   # (tests/test_gpu_packed_prefilter.py cyr)
    regex = {"1000": lambda: "|".join(latin), "3000": lambda: "|".join(W.keywords(3000, min_len=6, max_len=8)),
             "cyrillic": lambda: "|".join(cyr(w) for w in latin), "mixed": lambda: "|".join(W.keywords_mixed(300)),
             "unbounded": lambda: "(" + "|".join(latin) + ")[0-9]+", "digits": lambda: "[0-9]+",
             "nested": lambda: "international|inter|nation"}[kind]()
    return DFACompiler.compile(regex, "filter")


def routes(p):
    return [p.find_all_packed_route(cw, co) for cw in (1, 2) for co in (False, True)]


def test_symbol_is_exported(lib):
    from needle_amd import _lib
    assert hasattr(lib, "needle_pattern_find_all_packed_filter")
    assert "needle_pattern_find_all_packed_filter" in _lib.EXPORTS


def test_bad_arguments(lib):
    from needle_amd import _lib
    p = pattern("nested")
    a = ctypes.c_int32(-7)
    f = lib.needle_pattern_find_all_packed_filter
    assert f(None, 1, 0, ctypes.byref(a)) == _lib.ERR_INVALID
    assert f(p._h, 1, 0, None) == _lib.ERR_INVALID
    for cw in (0, 3, 4, -1):
        assert f(p._h, cw, 0, ctypes.byref(a)) == _lib.ERR_INVALID
    for co in (2, -1):
        assert f(p._h, 1, co, ctypes.byref(a)) == _lib.ERR_INVALID
    assert f(p._h, 1, 0, ctypes.byref(a)) == 0 and a.value == 0


@pytest.mark.parametrize("kind,modes", [("1000", (6,)), ("3000", (3, 5))])
def test_big_dictionaries_take_the_filter(lib, kind, modes):
    """1000 keywords of 6 .. 8 chars: the compressed automaton; 3000: hot rows / the HBM table."""
    p = pattern(kind)
    assert p.info()["kernel_mode"]["forwards"] in modes
    for cw in (1, 2):
        assert p.find_all_transducer(cw) is None
        for co in (False, True):
            assert p.find_all_packed_filter(cw, co) is True, (kind, cw, co)
    assert p.find_all_packed_filter() is True
    assert routes(p) == ROUTES_ALL_CONVERSION


def test_utf16_one_page_and_wide(lib):
    p = pattern("cyrillic")
    assert p.utf16_route() is not None and p.utf16_route()[0] == 4
    assert p.find_all_packed_filter(2) and p.find_all_packed_filter(2, True)
    assert routes(p) == ["lane", "conversion", "conversion", "conversion"]
    assert not p.find_all_packed_filter(1, False)     # (8-bit rows see the small automaton of the chars below 0x100: the per-lane kernel)
    p = pattern("mixed")
    assert p.utf16_route() is None
    assert p.find_all_packed_filter(2) and p.find_all_packed_filter(2, True)
    assert routes(p) == ROUTES_ALL_CONVERSION


@pytest.mark.parametrize("kind,route", [("digits", "transducer"), ("nested", "lane")])
def test_patterns_of_the_other_routes(lib, kind, route):
    p = pattern(kind)
    assert routes(p) == [route] * 4
    for cw in (1, 2):
        for co in (False, True):
            assert p.find_all_packed_filter(cw, co) is False, (kind, cw, co)


def test_big_pattern_without_bounded_match_lengths(lib):
    """`(1000 keywords)[0-9]+`: no lengths form, so the filter's find-all form has no program: conversion, as before."""
    p = pattern("unbounded")
    assert routes(p) == ROUTES_ALL_CONVERSION
    for cw in (1, 2):
        for co in (False, True):
            assert p.find_all_packed_filter(cw, co) is False, (cw, co)
