"""Spans of packed rows as a new packed batch on the device (needle_gather_spans_lengths_packed_dev / needle_gather_spans_fill_packed_dev /
needle_split_spans_packed_dev / needle_gather_matches_packed_host; Pattern.gather_spans_packed / split_spans_packed / extract_all_packed /
split_packed / select_rows_packed / grep_packed and the string and bytes conveniences): bit-exact against gather_ref / split_list_ref
(tests/gather_cases.py) of the oracle's lists, no tolerances.  Every device run writes into a buffer with 64 sentinel code units in front
of out_offsets[M0] and at least 64 behind out_offsets[M1]; they must come back untouched."""
import ctypes
import os
import random
import re
import subprocess
import sys

import numpy as np
import pytest

from gather_cases import clamp_span, flatten, gather_ref, packed_ref, split_list_ref
from test_gpu_configs import compiled
from test_gpu_find_all_packed import oracle_all
from test_gpu_packed_dev import device_packed, layout_rows
from test_gpu_replace_all import GUARD, LAYOUT_PATTERNS, check_guarded, guarded, units

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WHOLE = 0x7FFFFFFF  # a span end that the clamp turns into the row's length


def dev(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x)).to("cuda")


def check_gather(rows, lists, dtype, lead=5, trail=7, out_start=3, stream=None, junk=None, what=""):
    """gather_spans_packed (the two pattern-free entries) of a given list against gather_ref."""
    import torch
    from needle_amd.pattern import Pattern
    want, want_off, _ = packed_ref(rows, lists, dtype)
    data, offsets = device_packed(rows, dtype, lead=lead, trail=trail, junk=junk)
    so, st, en = flatten(lists)
    big, out, sent = guarded(want.size, out_start, dtype)
    got, out_off = Pattern.gather_spans_packed(data, offsets, dev(so), dev(st), dev(en), stream=stream, out=out, out_start=out_start)
    assert got.data_ptr() == out.data_ptr()
    torch.cuda.synchronize()
    check_guarded(big, sent, want, want_off, out_off, out_start, dtype, ("gather", what, "lead", lead, "out_start", out_start))


def check_pattern(p, rows, lists, dtype, lead=5, trail=7, junk=None, out_start=3, stream=None, what=""):
    """extract_all_packed and split_packed of the rows (device tensors) against the references of the oracle's lists."""
    import torch
    data, offsets = device_packed(rows, dtype, lead=lead, trail=trail, junk=junk)
    for name, run, spans in (("extract", p.extract_all_packed, lists), ("split", p.split_packed, split_list_ref(rows, lists))):
        want, want_off, want_so = packed_ref(rows, spans, dtype)
        if name == "split":
            assert want_off.size - 1 == sum(len(l) for l in lists) + len(rows), ("split rows", what)
        big, out, sent = guarded(want.size, out_start, dtype)
        got, out_off, so = run(data, offsets, stream=stream, out=out, out_start=out_start)
        assert got.data_ptr() == out.data_ptr()
        torch.cuda.synchronize()
        assert (so.cpu().numpy() == want_so).all(), ("span offsets", name, what)
        check_guarded(big, sent, want, want_off, out_off, out_start, dtype, (name, what, "lead", lead, "out_start", out_start))


@pytest.fixture(scope="module")
def layout_cases():
    """Per pattern: (pattern, oracle, dtype, rows, the oracle's lists, junk) -- the rows and the lists made once, shared by the tests."""
    cache = {}

    def get(regex, cw, alphabet, plants, junk):
        key = (regex, cw)
        if key not in cache:
            p, o = compiled(regex)
            dtype = np.uint8 if cw == 1 else np.uint16
            rng = np.random.default_rng(17 + len(regex) + cw)
            rows = layout_rows(rng, [ord(ch) for ch in alphabet], plants, n=700, max_len=120, dtype=dtype)
            cache[key] = (p, o, dtype, rows, oracle_all(o, rows), [ord(ch) for ch in junk])
        return cache[key]
    return get


@pytest.mark.gpu
@pytest.mark.parametrize("regex,cw,alphabet,plants,junk,ralpha", LAYOUT_PATTERNS)
def test_layouts(layout_cases, regex, cw, alphabet, plants, junk, ralpha):
    """1. Patterns x char widths x layouts x batch sizes, and only empty rows: extract and split."""
    p, o, dtype, rows, lists, jk = layout_cases(regex, cw, alphabet, plants, junk)
    assert sum(len(l) for l in lists) > 100
    check_pattern(p, rows, lists, dtype, lead=5, trail=7, junk=jk, out_start=3, what="lead 5 trail 7")
    check_pattern(p, rows, lists, dtype, lead=0, trail=0, junk=jk, out_start=64, what="offsets[0] = 0, out_offsets[0] = 64")
    check_pattern(p, rows, lists, dtype, lead=133, trail=0, junk=jk, out_start=3, what="offsets[0] > 0")
    for n in (1, 63, 64, 65, 130):
        check_pattern(p, rows[48:48 + n], lists[48:48 + n], dtype, lead=3, trail=5, junk=jk, what="n_rows %d" % n)
    empty = [np.zeros(0, dtype)] * 70
    check_pattern(p, empty, oracle_all(o, empty), dtype, lead=9, trail=9, junk=jk, what="70 empty rows")


@pytest.mark.gpu
@pytest.mark.parametrize("cw", [1, 2])
@pytest.mark.parametrize("out_start", range(16))
def test_alignment_sweep(cw, out_start):
    """2. One 40-unit row, every span (s, s + L), s in 0..15, L in 0..33: as 544 single-span lists -- each output is all edge, bordering the
    caller's memory on both sides -- and as one list of all of them: every source and destination misalignment mod 16."""
    import torch
    from needle_amd.pattern import Pattern
    dtype = np.uint8 if cw == 1 else np.uint16
    row = (np.arange(40) * 7 + 33).astype(dtype)
    spans = [(s, s + L) for s in range(16) for L in range(34)]
    data, offsets = device_packed([row], dtype, lead=5, trail=7, junk=[0x11])
    stride = 112  # a multiple of 16 code units: every call's output starts at out_start mod 16 and leaves sentinels to the next
    big, out, sent = guarded(len(spans) * stride, 0, dtype)
    want = np.full(big.numel(), sent, dtype)
    st, en = dev(np.array([s for s, _ in spans], np.int32)), dev(np.array([e for _, e in spans], np.int32))
    one = dev(np.array([0, 1], np.int64))
    offs = []
    for k, (s, e) in enumerate(spans):
        at = k * stride + out_start
        _, oo = Pattern.gather_spans_packed(data, offsets, one, st[k:k + 1], en[k:k + 1], out=out, out_start=at)
        offs.append(oo)
        s2, e2 = clamp_span(s, e, 40)
        want[GUARD + at:GUARD + at + (e2 - s2)] = row[s2:e2]
    torch.cuda.synchronize()
    got = big.cpu().numpy().view(dtype)
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, ("single-span lists", bad[:8], got[bad[:8]], want[bad[:8]])
    for k, (s, e) in enumerate(spans[::37]):
        s2, e2 = clamp_span(s, e, 40)
        assert offs[k * 37].tolist() == [k * 37 * stride + out_start, k * 37 * stride + out_start + e2 - s2]
    check_gather([row], [spans], dtype, lead=5, trail=7, out_start=out_start, what="all spans in one list")
    check_gather([row], [spans], dtype, lead=out_start, trail=(-(out_start + 40)) % (4 // cw), out_start=5, what="lead swept")


@pytest.mark.gpu
def test_pieces_per_block():
    """3. Sixteen one-byte spans in one 16-byte output block; empty spans alternating with one-unit spans; a list of empty spans only."""
    import torch
    from needle_amd.pattern import Pattern
    p, o = compiled("[0-9]")
    text = "".join("%d%s" % (i % 10, "abcdefg"[i % 7]) for i in range(150))
    rows = [units(text, np.uint8)] * 70
    lists = oracle_all(o, rows[:1]) * len(rows)
    assert len(lists[0]) == 150 and len(text) == 300
    check_pattern(p, rows, lists, np.uint8, what="1a2b3c")
    for dtype in (np.uint8, np.uint16):
        r = [units(text, dtype)] * 70
        hand = [[(i, i) if i % 2 else (i, i + 1) for i in range(300)]] * 70
        check_gather(r, hand, dtype, lead=2, trail=1, out_start=7, what="empty and one-unit spans")
        none = [[(i, i) for i in range(50)]] * 70
        so, st, en = flatten(none)
        data, offsets = device_packed(r, dtype)
        big, out, sent = guarded(0, 0, dtype)
        got, out_off = Pattern.gather_spans_packed(data, offsets, dev(so), dev(st), dev(en), out=out[:0])
        torch.cuda.synchronize()
        assert got.numel() == 0 and (out_off.cpu().numpy() == 0).all() and out_off.numel() == 70 * 50 + 1
        assert (big.cpu().numpy().view(dtype) == sent).all()
        got, out_off = Pattern.gather_spans_packed(data, offsets, dev(so), dev(st), dev(en))
        assert got.numel() == 0 and (out_off.cpu().numpy() == 0).all()


@pytest.mark.gpu
@pytest.mark.parametrize("n_rows", [64, 65])
def test_chunk_boundary(n_rows):
    """4. One 64-row group with K - 1, K, K + 1 and 2K + 3 spans (K: what the fill kernel tables at once), all in one row and spread."""
    from needle_amd import _lib
    K = _lib.lib().needle_gather_chunk_spans()
    assert K >= 64
    rng = np.random.default_rng(4)
    rows = [rng.integers(97, 123, int(k)).astype(np.uint8) for k in rng.integers(20, 60, n_rows)]
    span = lambda r: tuple(sorted(int(x) for x in rng.integers(0, len(rows[r]) + 1, 2)))
    for count in (K - 1, K, K + 1, 2 * K + 3):
        one_row = [[] for _ in rows]
        one_row[17] = [span(17) for _ in range(count)]
        spread = [[span(r) for _ in range(count // 64 + (r < count % 64))] if r < 64 else [span(r)] * 3 for r in range(n_rows)]
        assert sum(len(l) for l in spread[:64]) == count
        for dtype in (np.uint8, np.uint16):
            r = [x.astype(dtype) for x in rows]
            check_gather(r, one_row, dtype, what=("one row", count))
            check_gather(r, spread, dtype, lead=1, trail=2, out_start=9, what=("spread", count))


@pytest.mark.gpu
@pytest.mark.parametrize("cw", [1, 2])
def test_long_spans(cw):
    """5. Whole-row spans over rows of 1023 .. 5000 units among short rows: a span that covers more than one step of the wave, and more
    than two; the long rows in one group and in separate groups.  Every span is (0, 2^31 - 1): the clamp makes it the row."""
    dtype = np.uint8 if cw == 1 else np.uint16
    rng = np.random.default_rng(5 + cw)
    short = layout_rows(rng, list(range(97, 123)), [], n=330, max_len=30, dtype=dtype)
    longs = [rng.integers(65, 91, k).astype(dtype) for k in (1023, 1024, 1025, 1500, 5000)]
    for places in ((3, 10, 20, 30, 40), (5, 70, 135, 200, 265)):
        rows = list(short)
        for at, row in zip(places, longs):
            rows[at] = row
        check_gather(rows, [[(0, WHOLE)] for _ in rows], dtype, lead=3, trail=6, out_start=5, what=("whole rows", places))
        twice = [[(0, WHOLE), (1, len(r) - 1)] if len(r) > 1000 else [] for r in rows]
        check_gather(rows, twice, dtype, lead=0, trail=0, out_start=0, what=("long rows only", places))


def arbitrary_lists(rng, rows):
    lists = []
    for i, r in enumerate(rows):
        n, k = len(r), int(rng.integers(0, 7))
        l = []
        for _ in range(k):
            kind = int(rng.integers(0, 6))
            a, b = sorted(int(x) for x in rng.integers(0, n + 1, 2))
            l.append([(a, b), (b, a), (a - 9, b), (a, b + 50), (a, b), (-5, -1)][kind])
            if kind == 4:
                l.append((a, b))  # repeated
        lists.append(l)
    lists[77] = [(2, 11)] * 100  # the same span 100 times
    return lists


@pytest.mark.gpu
@pytest.mark.parametrize("cw", [1, 2])
def test_arbitrary_lists(cw):
    """6. Reversed, overlapping, repeated and out-of-row spans over 200 rows: defined by the clamp.  Then the list stored behind 37
    unrelated entries (span_offsets[0] = 37) on a non-default stream: lengths before M0 and from M1 on stay untouched."""
    import torch
    from needle_amd import _lib
    from needle_amd.pattern import Pattern
    dtype = np.uint8 if cw == 1 else np.uint16
    rng = np.random.default_rng(60 + cw)
    rows = layout_rows(rng, list(range(97, 123)), [], n=200, max_len=90, dtype=dtype)
    rows[77] = np.arange(20).astype(dtype) + 65
    lists = arbitrary_lists(rng, rows)
    check_gather(rows, lists, dtype, what="arbitrary")
    check_gather(rows, lists, dtype, lead=0, trail=0, out_start=64, what="arbitrary, offsets[0] = 0")
    # span_offsets[0] = 37
    want, want_off, _ = packed_ref(rows, lists, dtype)
    so, st, en = flatten(lists)
    m = st.size
    st2 = np.concatenate([np.full(37, 3, np.int32), st, np.full(5, 1, np.int32)])
    en2 = np.concatenate([np.full(37, 9, np.int32), en, np.full(5, 8, np.int32)])
    data, offsets = device_packed(rows, dtype, lead=5, trail=7)
    d_so, d_st, d_en = dev(so + 37), dev(st2), dev(en2)
    big, out, sent = guarded(want.size, 3, dtype)
    lens = dev(np.full(m + 42, 0xDEAD, np.int64))
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    _, out_off = Pattern.gather_spans_packed(data, offsets, d_so, d_st, d_en, stream=side.cuda_stream, out=out, out_start=3)
    v = _lib.PackedView()
    v.data, v.char_width, v.n_rows, v.offsets = data.data_ptr(), cw, len(rows), offsets.data_ptr()
    assert _lib.lib().needle_gather_spans_lengths_packed_dev(ctypes.byref(v), d_so.data_ptr(), d_st.data_ptr(), d_en.data_ptr(), lens.data_ptr(),
                                                             side.cuda_stream) == 0
    side.synchronize()
    oo = out_off.cpu().numpy()
    assert oo.size == m + 43 and (oo[:37] == 3).all() and (oo[37 + m:] == 3 + want.size).all()
    check_guarded(big, sent, want, want_off, out_off[37:37 + m + 1], 3, dtype, "list behind 37 entries, side stream")
    got = lens.cpu().numpy()
    assert (got[:37] == 0xDEAD).all() and (got[37 + m:] == 0xDEAD).all() and (got[37:37 + m] == np.diff(want_off)).all()


@pytest.mark.gpu
@pytest.mark.parametrize("cw", [1, 2])
def test_wrong_out_offsets(cw):
    """7. out_offsets that are not the prefix sum of the lengths -- all equal; half the true lengths -- give unspecified text and never a
    write outside [out_offsets[M0], out_offsets[M1]): only the sentinels are checked.  The offsets stay inside the buffer."""
    import torch
    from needle_amd import _lib
    dtype = np.uint8 if cw == 1 else np.uint16
    rng = np.random.default_rng(70 + cw)
    rows = layout_rows(rng, list(range(97, 123)), [], n=200, max_len=90, dtype=dtype)
    lists = arbitrary_lists(rng, rows)
    want, want_off, _ = packed_ref(rows, lists, dtype)
    so, st, en = flatten(lists)
    data, offsets = device_packed(rows, dtype, lead=5, trail=7)
    d_so, d_st, d_en = dev(so), dev(st), dev(en)
    v = _lib.PackedView()
    v.data, v.char_width, v.n_rows, v.offsets = data.data_ptr(), cw, len(rows), offsets.data_ptr()
    half = np.zeros_like(want_off)
    half[1:] = np.cumsum(np.diff(want_off) // 2)
    for name, off in (("all equal", np.zeros_like(want_off)), ("half the lengths", half)):
        for out_start in (0, 5):
            big, out, sent = guarded(want.size, out_start, dtype)
            d_oo = dev(off + out_start)
            assert _lib.lib().needle_gather_spans_fill_packed_dev(ctypes.byref(v), d_so.data_ptr(), d_st.data_ptr(), d_en.data_ptr(), d_oo.data_ptr(),
                                                                  out.data_ptr(), None) == 0
            torch.cuda.synchronize()
            got = big.cpu().numpy().view(dtype)
            a, b = GUARD + out_start + int(off[0]), GUARD + out_start + int(off[-1])
            assert (got[:a] == sent).all() and (got[b:] == sent).all(), (name, out_start)


@pytest.mark.gpu
@pytest.mark.parametrize("cw", [1, 2])
def test_select_and_grep(cw):
    """8. The rows a bitmap selects: none, all (the text as it is, the offsets rebased), seeded random -- as bool and as bitmap words --
    and grep_packed against the oracle's contained_in; 700 and 130 rows (no multiple of 64)."""
    import torch
    from needle_amd.pattern import Pattern
    dtype = np.uint8 if cw == 1 else np.uint16
    p, o = compiled("[0-9]+")
    rng = np.random.default_rng(80 + cw)
    rows = layout_rows(rng, [ord(ch) for ch in "abcxyz 0123456789"], [], n=700, max_len=60, dtype=dtype)
    for n in (700, 130):
        rs = rows[:n]
        data, offsets = device_packed(rs, dtype, lead=5, trail=7, junk=[ord("7")])
        contained = np.array([o.contained_in(r) for r in rs])
        assert 0 < contained.sum() < n
        for name, sel in (("none", np.zeros(n, bool)), ("all", np.ones(n, bool)), ("random", rng.random(n) < 0.4), ("grep", contained)):
            lists = [[(0, len(r))] if s else [] for r, s in zip(rs, sel)]
            want, want_off, _ = packed_ref(rs, lists, dtype)
            words = np.packbits(np.concatenate([sel, np.zeros((-n) % 64, bool)]), bitorder="little").view(np.int64)
            for bits in (dev(sel), dev(words)):
                big, out, sent = guarded(want.size, 3, dtype)
                if name == "grep":
                    _, out_off = p.grep_packed(data, offsets, out=out, out_start=3)
                else:
                    _, out_off = Pattern.select_rows_packed(data, offsets, bits, out=out, out_start=3)
                torch.cuda.synchronize()
                check_guarded(big, sent, want, want_off, out_off, 3, dtype, (name, n, str(bits.dtype)))
            if name == "all":
                text, off = Pattern.select_rows_packed(data, offsets, dev(sel))
                lo, hi = int(offsets[0]), int(offsets[-1])
                assert torch.equal(text, data[lo:hi]) and torch.equal(off, offsets - lo)
    # numpy inputs are uploaded and the result brought back
    hd, ho = data.cpu().numpy().view(dtype), offsets.cpu().numpy()
    got, got_off = p.grep_packed(hd, ho)
    assert got.dtype == dtype and (got == want).all() and (got_off == want_off).all()
    got, got_off = Pattern.select_rows_packed(hd, ho, contained)
    assert (got == want).all() and (got_off == want_off).all()


@pytest.mark.gpu
def test_chain(layout_cases):
    """9. The extracted batch is a packed view for every entry: each of its rows matches the pattern that found it, and a set's masks of
    its rows are the masks the set gives the spans of the original list."""
    import torch
    from needle_amd.pattern import DFACompiler, PatternSet, unpack_bitmap
    for case in (LAYOUT_PATTERNS[2], LAYOUT_PATTERNS[3]):
        regex, cw, alphabet, plants, junk, _ = case
        p, o, dtype, rows, lists, jk = layout_cases(regex, cw, alphabet, plants, junk)
        data, offsets = device_packed(rows, dtype, lead=5, trail=7, junk=jk)
        text, off, so = p.extract_all_packed(data, offsets)
        m = off.numel() - 1
        assert m == sum(len(l) for l in lists) > 100
        assert unpack_bitmap(p.matches_packed(text, off), m).all()
        ps = PatternSet([DFACompiler.compile(r) for r in ("abc+d", "ab", "[a-c]+", "abcd")])
        moff, st, en, tags = ps.tag_matches_packed(p, data, offsets)
        masks = ps.matches_packed(text, off)
        torch.cuda.synchronize()
        assert torch.equal(moff, so) and torch.equal(masks, tags) and (tags.cpu().numpy() != 0).all()
        assert len(set(tags.cpu().numpy().tolist())) > 1


HOST_CHILD = r'''
import sys
sys.path.insert(0, "."); sys.path.insert(0, "tests")
import test_gpu_gather as T
T.host_entry_checks()
print("HOST-GATHER-OK")
'''


def host_entry_checks():
    """extract_all_strings / split_strings, the packed entry on 8-bit rows with offsets that start above 0, and the capacity protocol of
    needle_gather_matches_packed_host, against the references of the oracle's lists."""
    from needle_amd import _lib
    from needle_amd.pattern import pack_strings
    from test_gpu_replace_all import host_strings
    p, o = compiled("[0-9]+")
    strings = host_strings()
    lists = [o.find_all(s, limit=1 << 30) for s in strings]
    pieces = split_list_ref(strings, lists)
    assert p.extract_all_strings(strings) == gather_ref(strings, lists)
    assert p.split_strings(strings) == gather_ref(strings, pieces)
    assert p.grep_strings(strings) == [s for s, l in zip(strings, lists) if l]
    # the packed entry through numpy arrays, 8-bit rows, offsets[0] > 0 and junk around the rows; the device route gives the same
    rows = [np.frombuffer(s.encode("ascii", "replace"), np.uint8) for s in strings]
    lists8 = oracle_all(o, rows)
    data, offsets = device_packed(rows, np.uint8, lead=37, trail=9, junk=[ord("5")])
    hd, ho = data.cpu().numpy(), offsets.cpu().numpy()
    assert ho[0] >= 37
    for run, spans in ((p.extract_all_packed, lists8), (p.split_packed, split_list_ref(rows, lists8))):
        want, want_off, want_so = packed_ref(rows, spans, np.uint8)
        got, got_off, got_so = run(hd, ho)
        assert got.dtype == np.uint8 and (got == want).all() and (got_off == want_off).all() and (got_so == want_so).all()
        got, got_off, got_so = run(data, offsets)
        assert (got.cpu().numpy() == want).all() and (got_off.cpu().numpy() == want_off).all() and (got_so.cpu().numpy() == want_so).all()
    # the capacity protocol on the raw entry, 16-bit rows, both modes
    L = _lib.lib()
    data16, off16 = pack_strings(strings)
    rows16 = [units(s, np.uint16) for s in strings]
    v = _lib.PackedView()
    v.data, v.char_width, v.n_rows, v.offsets = data16.ctypes.data, 2, len(strings), off16.ctypes.data
    for mode, spans in ((_lib.GATHER_MATCHES, lists), (_lib.GATHER_PIECES, pieces)):
        want, want_off, want_so = packed_ref(rows16, spans, np.uint16)
        ns, nu = want_off.size - 1, want.size
        span_off = np.full(len(strings) + 1, 99, np.uint64)
        tot_s, tot_u = ctypes.c_uint64(0), ctypes.c_uint64(0)

        def call(out_off, span_cap, text, unit_cap):
            span_off[:] = 99
            rc = L.needle_gather_matches_packed_host(p._h, ctypes.byref(v), mode, span_off.ctypes.data, out_off.ctypes.data if out_off is not None else None,
                                                     span_cap, text.ctypes.data if text is not None else None, unit_cap, ctypes.byref(tot_s),
                                                     ctypes.byref(tot_u))
            assert rc == 0 and tot_s.value == ns and tot_u.value == nu and (span_off.astype(np.int64) == want_so).all(), (mode, span_cap, unit_cap)
        call(None, 0, None, 0)                                                 # sizes only
        oo, text = np.full(ns + 1 + 16, 77, np.uint64), np.full(nu + 16, 0xA5A5, np.uint16)
        call(oo, ns - 1, text, nu)                                             # one output row short
        assert (oo[ns:] == 77).all() and (text[nu:] == 0xA5A5).all()
        oo[:], text[:] = 77, 0xA5A5
        call(oo, ns, text, nu - 1)                                             # one code unit short
        assert (oo[ns + 1:] == 77).all() and (text[nu - 1:] == 0xA5A5).all()
        oo[:], text[:] = 77, 0xA5A5
        call(oo, ns, text, nu)                                                 # exact
        assert (oo[:ns + 1].astype(np.int64) == want_off).all() and (oo[ns + 1:] == 77).all()
        assert (text[:nu] == want).all() and (text[nu:] == 0xA5A5).all()


@pytest.mark.gpu
def test_host_entry():
    """10. The host entry: 2000 mixed-length strings in one chunk (here) and in several (a child process: NEEDLE_HOST_CHUNK_BYTES and
    NEEDLE_HOST_RESULT_BYTES are read once per process), both modes and widths, the capacity protocol, offsets that start above 0."""
    host_entry_checks()
    env = dict(os.environ, NEEDLE_HOST_CHUNK_BYTES="20000", NEEDLE_HOST_RESULT_BYTES="4096")
    r = subprocess.run([sys.executable, "-c", HOST_CHILD], env=env, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert "HOST-GATHER-OK" in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]


@pytest.mark.gpu
def test_utf8_bytes():
    """11. extract_all_bytes / split_bytes on UTF-8 rows with 2-, 3- and 4-byte sequences and ill-formed bytes: the references applied to
    find_all_bytes' byte positions; for well-formed rows also re on the decoded strings."""
    p, o = compiled("[0-9]+|中文|é+")
    rx = re.compile("[0-9]+|中文|é+")
    rng = random.Random(11)
    atoms = ["12", "7", "é", "éé", "中文", "中", "a", " b", "😀", "λ", "x9"]
    good = ["".join(rng.choice(atoms) for _ in range(rng.randint(0, 30))) for _ in range(300)]
    rows = [s.encode("utf-8") for s in good]
    bad = [b"\xff12\xc3", b"\xe4\xb8 45", b"12\xf0\x9f\x98", b"\xc3\xa9\xc3", b"\x80\x80 7 \xed\xa0\x80 88", b""]
    for i in range(200):
        b = bytearray(rng.choice(rows))
        for _ in range(rng.randint(1, 3)):
            if b:
                b[rng.randrange(len(b))] = rng.choice([0xFF, 0x80, 0xC3, 0xE4, 0xF0, 0x31])
        bad.append(bytes(b))
    for batch in (rows, bad, rows + bad):
        pos = p.find_all_bytes(batch)
        assert p.extract_all_bytes(batch) == gather_ref(batch, pos)
        assert p.split_bytes(batch) == gather_ref(batch, split_list_ref(batch, pos))
    assert [[x.decode("utf-8") for x in l] for l in p.extract_all_bytes(rows)] == [rx.findall(s) for s in good]
    assert [[x.decode("utf-8") for x in l] for l in p.split_bytes(rows)] == [rx.split(s) for s in good]
    assert sum(len(rx.findall(s)) for s in good) > 300


FUZZ_ALPHABET = [ord(c) for c in "abcxyz019 AB_\n."] + [0xE9, 0x416, 0x4E2D, 0xFFFF]


@pytest.mark.gpu
@pytest.mark.parametrize("seed", range(30))
def test_fuzz(seed):
    """12. A seeded random regex that does not match the empty string (drawn as the find-all fuzz tests draw theirs), 300 rows of at most
    200 units, both widths, random lead and out_start: extract and split against the references of the oracle's lists."""
    from needle_amd.pattern import PatternException
    from test_compile_vs_python_restatement import FLAG_SETS, random_regex
    rng = random.Random(9100 + seed)
    nrng = np.random.default_rng(seed)
    while True:
        regex, flags = random_regex(rng), rng.choice(FLAG_SETS)
        try:
            p, o = compiled(regex, flags)
        except (PatternException, ValueError):
            continue
        if not o.matches(""):
            break
    rows16 = layout_rows(nrng, FUZZ_ALPHABET, [], n=300, max_len=200, dtype=np.uint16)
    check_pattern(p, rows16, oracle_all(o, rows16), np.uint16, lead=int(nrng.integers(0, 9)), trail=int(nrng.integers(0, 2)) * 5, junk=FUZZ_ALPHABET,
                  out_start=int(nrng.integers(0, 40)), what=(regex, flags))
    small = [c for c in FUZZ_ALPHABET if c < 256]
    rows8 = layout_rows(nrng, small, [], n=300, max_len=200)
    check_pattern(p, rows8, oracle_all(o, rows8), np.uint8, lead=int(nrng.integers(0, 9)), trail=3, junk=small, out_start=int(nrng.integers(0, 40)),
                  what=(regex, flags))
