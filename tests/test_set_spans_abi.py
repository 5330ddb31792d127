"""Tags for a match list on the CPU (needle_set_matches_spans_packed_dev, needle_set_tag_matches_packed_host; the Python surface of
PatternSet around them): the symbols and their argument checks without a device, union_pattern() / first_member(), and a check of the
GPU tests' own inputs -- the union spans of the batch recipe carry every member's bit, and the oracle's per-span masks are what the
set's product tables give on the substrings."""
import ctypes
import inspect

import numpy as np
import pytest

from pattern_set_cases import SETS, compile_set, walk_tables
from set_spans_cases import SHADOWED, clamp_span, reference_span_masks, union_regex, union_spans

VP, U64 = ctypes.c_void_p, ctypes.c_uint64


@pytest.fixture(scope="module")
def lib():
    from needle_amd import build
    build.build()
    from oracle import walker
    walker.build()
    from needle_amd import _lib
    return _lib.lib()


def test_symbols_and_signatures(lib):
    from needle_amd import _lib
    from needle_amd.pattern import PatternSet
    for n in ("needle_set_matches_spans_packed_dev", "needle_set_tag_matches_packed_host"):
        assert n in _lib.EXPORTS and hasattr(lib, n), n
    P = ctypes.POINTER
    assert lib.needle_set_matches_spans_packed_dev.argtypes == [VP, P(_lib.PackedView), VP, VP, VP, VP, VP]
    assert lib.needle_set_tag_matches_packed_host.argtypes == [VP, VP, P(_lib.PackedView), VP, VP, VP, VP, U64, P(U64)]
    sig = lambda f: list(inspect.signature(f).parameters)
    assert sig(PatternSet.matches_spans_packed) == ["self", "data", "offsets", "span_offsets", "start", "end", "stream", "out"]
    assert sig(PatternSet.tag_matches_packed) == ["self", "pattern", "data", "offsets", "stream"]
    assert sig(PatternSet.find_all_tagged_strings) == ["self", "pattern", "strings"]
    assert sig(PatternSet.first_member) == ["masks"] and sig(PatternSet.union_pattern) == ["self"]


def test_argument_checks_need_no_device(lib):
    from needle_amd import _lib
    from needle_amd.pattern import DFACompiler, PatternSet
    ps = PatternSet([DFACompiler.compile("[0-9]+", "d"), DFACompiler.compile("ab", "e")])
    pat = DFACompiler.compile("[0-9]+|ab", "u")
    data = np.frombuffer(b"ab12cd..", dtype=np.uint8).copy()
    offsets = np.array([0, 4, 6], dtype=np.uint64)
    span_off = np.array([0, 2, 2], dtype=np.uint64)
    start, end = np.array([0, 2], dtype=np.int32), np.array([2, 4], dtype=np.int32)
    masks = np.zeros(2, dtype=np.uint32)

    def view(data_ptr=data.ctypes.data, cw=1, n=2, off=offsets.ctypes.data):
        v = _lib.PackedView()
        v.data, v.char_width, v.n_rows, v.offsets = data_ptr, cw, n, off
        return v
    fn = lib.needle_set_matches_spans_packed_dev
    so, st, en, mk = span_off.ctypes.data, start.ctypes.data, end.ctypes.data, masks.ctypes.data
    assert fn(None, ctypes.byref(view()), so, st, en, mk, None) == _lib.ERR_INVALID            # NULL set
    assert fn(ps._h, None, so, st, en, mk, None) == _lib.ERR_INVALID                           # NULL view
    assert fn(ps._h, ctypes.byref(view(off=None)), so, st, en, mk, None) == _lib.ERR_INVALID   # NULL offsets
    assert fn(ps._h, ctypes.byref(view()), None, st, en, mk, None) == _lib.ERR_INVALID         # NULL span offsets
    assert fn(ps._h, ctypes.byref(view()), so, st, en, None, None) == _lib.ERR_INVALID         # NULL masks
    assert fn(ps._h, ctypes.byref(view(cw=3)), so, st, en, mk, None) == _lib.ERR_INVALID       # bad char_width
    assert fn(ps._h, ctypes.byref(view(data_ptr=data.ctypes.data + 1)), so, st, en, mk, None) == _lib.ERR_INVALID  # not 4-byte aligned
    assert fn(ps._h, ctypes.byref(view(n=0)), so, None, None, mk, None) == _lib.NEEDLE_OK      # an empty batch
    assert not masks.any()
    host = lib.needle_set_tag_matches_packed_host
    out_off, total = np.zeros(3, dtype=np.uint64), U64(7)
    args = (out_off.ctypes.data, st, en, mk)
    assert host(None, pat._h, ctypes.byref(view()), *args, 2, ctypes.byref(total)) == _lib.ERR_INVALID           # NULL set
    assert host(ps._h, None, ctypes.byref(view()), *args, 2, ctypes.byref(total)) == _lib.ERR_INVALID            # NULL pattern
    assert host(ps._h, pat._h, None, *args, 2, ctypes.byref(total)) == _lib.ERR_INVALID                          # NULL view
    assert host(ps._h, pat._h, ctypes.byref(view(cw=0)), *args, 2, ctypes.byref(total)) == _lib.ERR_INVALID      # bad char_width
    assert host(ps._h, pat._h, ctypes.byref(view()), None, st, en, mk, 2, ctypes.byref(total)) == _lib.ERR_INVALID  # NULL offsets out
    assert host(ps._h, pat._h, ctypes.byref(view()), *args, 2, None) == _lib.ERR_INVALID                         # NULL total
    assert host(ps._h, pat._h, ctypes.byref(view()), out_off.ctypes.data, st, en, None, 2, ctypes.byref(total)) == _lib.ERR_INVALID  # NULL masks, capacity > 0
    assert host(ps._h, pat._h, ctypes.byref(view(n=0)), out_off.ctypes.data, None, None, None, 0, ctypes.byref(total)) == _lib.NEEDLE_OK
    assert total.value == 0
    # a valid call: NEEDLE_ERR_DEVICE where there is no device.  (The _dev entry takes DEVICE pointers: it is called with these host
    # arrays only where no device can follow them.)
    no_device = lib.needle_device_count() <= 0
    rc = host(ps._h, pat._h, ctypes.byref(view()), *args, 2, ctypes.byref(total))
    assert rc == (_lib.ERR_DEVICE if no_device else _lib.NEEDLE_OK), (rc, lib.needle_last_error())
    if no_device:
        assert fn(ps._h, ctypes.byref(view()), so, st, en, mk, None) == _lib.ERR_DEVICE
    else:
        assert total.value == 2 and masks.tolist() == [2, 1] and start.tolist() == [0, 2] and end.tolist() == [2, 4]


@pytest.mark.parametrize("name", ["nullable4", "logs8", "u16b"])
def test_union_pattern_compiles(lib, name):
    ps, _, _ = compile_set(name)
    assert ps.members == [(p, 0) for p in SETS[name][0]]
    u = ps.union_pattern()
    assert u.regex == union_regex(name) and u.flags == 0


def test_union_pattern_refuses_mixed_flags_and_table_members(lib):
    from needle_amd.pattern import CASE_INSENSITIVE, DFACompiler, Pattern, PatternSet
    a, b = DFACompiler.compile("ab", "a", 0), DFACompiler.compile("cd", "b", CASE_INSENSITIVE)
    with pytest.raises(ValueError):
        PatternSet([a, b]).union_pattern()
    both = PatternSet([DFACompiler.compile("ab", "a", CASE_INSENSITIVE), b]).union_pattern()
    assert both.flags == CASE_INSENSITIVE and both.regex == "(ab)|(cd)"
    with pytest.raises(ValueError):  # a member without a regex source
        PatternSet([a, Pattern.from_bytes(a.to_bytes())]).union_pattern()


def test_first_member():
    from needle_amd.pattern import PatternSet
    masks = np.array([0, 1, 2, 3, 0x80000000, 0x80000001, 0x00010000, 0xFFFFFFFF, 0x6], dtype=np.uint32)
    want = [-1, 0, 1, 0, 31, 0, 16, 0, 1]
    assert PatternSet.first_member(masks).tolist() == want
    assert PatternSet.first_member(masks.view(np.int32)).tolist() == want  # (the device entries' int32 tensors: bit 31 is the sign)
    assert PatternSet.first_member(np.array([1 << i for i in range(32)], dtype=np.uint32)).tolist() == list(range(32))
    assert PatternSet.first_member(np.zeros(0, np.uint32)).size == 0


@pytest.mark.parametrize("name", ["logs8", "u16b"])
def test_union_spans_carry_every_member_and_equal_the_product_tables(lib, name):
    """The GPU tests' input: every union span of the batch recipe has a non-zero reference mask, every member's bit occurs at least 3
    times -- but for the members that the reference's ordered alternation shadows (set_spans_cases.SHADOWED), whose bit no union span
    can carry -- and the oracle's masks are what PatternSet.tables("matches") gives on the substrings, ORed over the groups."""
    ps, oracles, dtype = compile_set(name)
    rows, spans = union_spans(name)
    off, start, end = spans
    want = reference_span_masks(oracles, rows, spans)
    assert want.size >= 3 * len(oracles) and (want != 0).all(), np.nonzero(want == 0)[0][:10]
    for i in range(len(oracles)):
        c = int(((want >> np.uint32(i)) & 1).sum())
        assert c == 0 if i in SHADOWED.get(name, ()) else c >= 3, (name, i, c)
    for i in SHADOWED.get(name, ()):  # ... whose bit the whole-row spans carry instead
        assert sum(1 for r in rows if oracles[i].matches(np.ascontiguousarray(r))) >= 3, (name, i)
    cw = np.dtype(dtype).itemsize
    groups = [ps.tables("matches", cw, g) for g in range(ps.info("matches", cw)["n_groups"])]
    for r, row in enumerate(rows):
        for m in range(int(off[r]), int(off[r + 1])):
            s, e = clamp_span(start[m], end[m], len(row))
            got = 0
            for t in groups:
                got |= walk_tables(t, row[s:e], "matches")
            assert got == int(want[m]), (name, r, m, s, e, got, int(want[m]))
