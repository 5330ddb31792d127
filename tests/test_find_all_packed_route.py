"""needle_pattern_find_all_packed_route / Pattern.find_all_packed_route: which route the packed find-all entries
(needle_count_matches_packed_dev, needle_find_all_csr_packed_dev) take for a pattern -- the transducer kernel, the per-lane kernel
(patterns without a transducer: nullable, unbounded with backward walks, nested dictionaries) or conversion.  Answered on the host:
no GPU here."""
import ctypes

import pytest

TRANSDUCER = ["[0-9]+", "abc|de"]
LANE = ["international|inter|nation", "[a-c]*", "http://.+", "abc+d|ab", "ab" + "c" * 300 + "d|ab", "[a-z一-丠]+[0-9]|ЖЗ+"]


@pytest.fixture(scope="module")
def lib():
    from needle_amd import build
    build.build()
    from needle_amd import _lib
    return _lib.lib()


def compile_(regex):
    from needle_amd.pattern import DFACompiler
    return DFACompiler.compile(regex, "route")


def test_symbol_is_exported(lib):
    from needle_amd import _lib
    assert hasattr(lib, "needle_pattern_find_all_packed_route")
    assert "needle_pattern_find_all_packed_route" in _lib.EXPORTS


def test_bad_arguments(lib):
    from needle_amd import _lib
    p = compile_("abc+d|ab")
    route = ctypes.c_int32(-7)
    f = lib.needle_pattern_find_all_packed_route
    assert f(None, 1, 0, ctypes.byref(route)) == _lib.ERR_INVALID
    assert f(p._h, 1, 0, None) == _lib.ERR_INVALID
    for cw in (0, 3, 4, -1):
        assert f(p._h, cw, 0, ctypes.byref(route)) == _lib.ERR_INVALID
    for co in (2, -1):
        assert f(p._h, 1, co, ctypes.byref(route)) == _lib.ERR_INVALID
    assert f(p._h, 1, 0, ctypes.byref(route)) == 0 and route.value == 2


@pytest.mark.parametrize("regex", TRANSDUCER)
def test_transducer_patterns(lib, regex):
    p = compile_(regex)
    for cw in (1, 2):
        assert p.find_all_transducer(cw) is not None
        for co in (False, True):
            assert p.find_all_packed_route(cw, co) == "transducer", (regex, cw, co)


@pytest.mark.parametrize("regex", LANE)
def test_lane_patterns(lib, regex):
    p = compile_(regex)
    for cw in (1, 2):
        assert p.find_all_transducer(cw) is None, (regex, cw)
        for co in (False, True):
            assert p.find_all_packed_route(cw, co) == "lane", (regex, cw, co)
    assert p.find_all_packed_route() == "lane"
