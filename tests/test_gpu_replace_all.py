"""Replace every match of every packed row on the device (needle_replace_all_lengths_packed_dev / needle_replace_all_fill_packed_dev /
needle_replace_all_packed_host; Pattern.replace_all_packed / replace_first_packed / splice_packed / replace_all_strings): bit-exact
against splice(row, oracle.find_all(row), repl) (tests/test_replace_abi.py), no tolerances.  Every device run writes into a buffer with
at least 64 sentinel code units in front of out_offsets[0] and 64 behind out_offsets[n]; they must come back untouched."""
import os
import subprocess
import sys

import numpy as np
import pytest

from test_gpu_configs import compiled
from test_gpu_find_all_packed import oracle_all
from test_gpu_packed_dev import device_packed, layout_rows
from test_replace_abi import splice

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 64  # sentinel code units on either side


def units(s, dtype):
    return np.array([ord(ch) for ch in s], dtype=dtype)


def flatten(lists):
    off = np.zeros(len(lists) + 1, np.int64)
    off[1:] = np.cumsum([len(x) for x in lists])
    st = np.array([s for x in lists for s, _ in x], np.int32)
    en = np.array([e for x in lists for _, e in x], np.int32)
    return off, st, en


def expected(rows, lists, repl, dtype):
    """(the result text, its offsets from 0) by the reference splice."""
    out = [splice(np.asarray(r, dtype), l, repl) for r, l in zip(rows, lists)]
    off = np.zeros(len(rows) + 1, np.int64)
    off[1:] = np.cumsum([len(x) for x in out])
    return (np.concatenate(out) if out else np.zeros(0, dtype)).astype(dtype), off


def guarded(total, out_start, dtype):
    """A device buffer of sentinels: GUARD units, then the `out` view the entries get -- out_start more sentinels, the result, GUARD more."""
    import torch
    cw = np.dtype(dtype).itemsize
    sent = 0xA5 if cw == 1 else 0xA5A5
    size = GUARD + out_start + total + GUARD
    size += (-size * cw) % 4 // cw
    host = np.full(size, sent, dtype)
    big = torch.from_numpy(host.view(np.uint8) if cw == 1 else host.view(np.int16)).to("cuda")
    return big, big[GUARD:], sent


def check_guarded(big, sent, want, want_off, out_off, out_start, dtype, what):
    got = big.cpu().numpy().view(dtype)
    a, b = GUARD + out_start, GUARD + out_start + want.size
    assert (out_off.cpu().numpy() == want_off + out_start).all(), ("offsets", what)
    assert (got[:a] == sent).all(), ("sentinels in front", what, np.nonzero(got[:a] != sent)[0][:8])
    assert (got[b:] == sent).all(), ("sentinels behind", what, np.nonzero(got[b:] != sent)[0][:8] + b)
    bad = np.nonzero(got[a:b] != want)[0]
    assert bad.size == 0, ("text", what, bad[:8], got[a:b][bad[:8]], want[bad[:8]])


def check_replace(p, rows, lists, repl, dtype, lead=5, trail=7, junk=None, out_start=3, stream=None, what=""):
    """replace_all_packed of the rows (device tensors) against the reference splice of the oracle's lists."""
    import torch
    want, want_off = expected(rows, lists, repl, dtype)
    data, offsets = device_packed(rows, dtype, lead=lead, trail=trail, junk=junk)
    big, out, sent = guarded(want.size, out_start, dtype)
    got, out_off = p.replace_all_packed(data, offsets, repl, stream=stream, out=out, out_start=out_start)
    assert got.data_ptr() == out.data_ptr()
    torch.cuda.synchronize()
    check_guarded(big, sent, want, want_off, out_off, out_start, dtype, (what, "repl", len(repl), "lead", lead, "out_start", out_start))


def check_splice(rows, lists, repl, dtype, lead=5, trail=7, out_start=3, no_lists=False, what=""):
    """splice_packed (the two pattern-free entries) on a given list."""
    import torch
    from needle_amd.pattern import Pattern
    want, want_off = expected(rows, lists, repl, dtype)
    data, offsets = device_packed(rows, dtype, lead=lead, trail=trail)
    moff, st, en = flatten(lists)
    dev = lambda x: torch.from_numpy(x).to("cuda")
    if no_lists:
        assert st.size == 0
    big, out, sent = guarded(want.size, out_start, dtype)
    _, out_off = Pattern.splice_packed(data, offsets, dev(moff), dev(st), dev(en), repl, out=out, out_start=out_start)
    torch.cuda.synchronize()
    check_guarded(big, sent, want, want_off, out_off, out_start, dtype, (what, "repl", len(repl), "lead", lead, "out_start", out_start))


LAYOUT_PATTERNS = [
    # (regex, char width, alphabet, planted words, junk that matches, replacement alphabet)
    ("[0-9]+", 1, "abcxyz 0123456789", [], "0123", "#*<>"),
    ("[0-9]+", 2, "abcxyz 0123456789", [], "0123", "#*<>"),
    ("abc+d|ab", 1, "abcd ", ["abcd", "abcccd", "ab"], "abcd", "#*<>"),
    ("abc+d|ab", 2, "abcd ", ["abcd", "abcccd", "ab"], "abcd", "#*<>"),
    ("international|inter|nation", 1, "interntiol ", ["international", "inter", "nation"], "inter", "#*<>"),
    ("international|inter|nation", 2, "interntiol ", ["international", "inter", "nation"], "inter", "#*<>"),
    ("[a-c]*", 1, "abcd", [], "abc", "#*<>"),
    ("[a-c]*", 2, "abcd", [], "abc", "#*<>"),
    ("[α-ω]{2}[α-ω]*|ЖЗ+|中文", 2, "ab αβωЖЗ中文字", ["αβγ", "ЖЗЗ", "中文"], "αβγ", "猫λЖ→"),
]
REPL_LENGTHS = (0, 1, 3, 17, 4096)


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
    """1. Patterns x replacement lengths x char widths x layouts x batch sizes, and only empty rows."""
    p, o, dtype, rows, lists, jk = layout_cases(regex, cw, alphabet, plants, junk)
    assert sum(len(l) for l in lists) > 100
    for k in REPL_LENGTHS:
        repl = np.resize(units(ralpha, dtype), k)
        check_replace(p, rows, lists, repl, dtype, lead=5, trail=7, junk=jk, out_start=3, what="lead 5 trail 7")
        check_replace(p, rows, lists, repl, dtype, lead=0, trail=0, junk=jk, out_start=64, what="offsets[0] = 0, out_offsets[0] = 64")
        check_replace(p, rows, lists, repl, dtype, lead=133, trail=0, junk=jk, out_start=3, what="offsets[0] > 0")
        for n in (1, 63, 65, 130):
            check_replace(p, rows[48:48 + n], lists[48:48 + n], repl, dtype, lead=3, trail=5, junk=jk, what="n_rows %d" % n)
        empty = [np.zeros(0, dtype)] * 70
        check_replace(p, empty, oracle_all(o, empty), repl, dtype, lead=9, trail=9, junk=jk, what="70 empty rows")


@pytest.mark.gpu
@pytest.mark.parametrize("row", ["x", "xy"])
def test_shared_edges(row):
    """2. 200 one-match rows: the groups' output spans meet at every alignment inside a dword and inside a 16-byte block, on the input
    side (lead) and on the output side (out_offsets[0]); with "" every output span is empty ("x") or one char per row ("xy")."""
    p, o = compiled("x")
    rows = [units(row, np.uint8)] * 200
    lists = oracle_all(o, rows)
    assert all(l == [(0, 1)] for l in lists)
    for repl in ("abc", "", "ab"):
        r = units(repl, np.uint8)
        for lead in range(16):
            trail = (-(lead + 200 * len(row))) % 4  # (so that device_packed keeps the lead as it is)
            for out_start in range(16):
                check_splice(rows, lists, r, np.uint8, lead=lead, trail=trail, out_start=out_start, what=("edges", row, repl))
    check_replace(p, rows, lists, units("abc", np.uint8), np.uint8, lead=1, trail=0, out_start=5, what="edges through the pattern")


@pytest.mark.gpu
def test_more_matches_than_a_chunk():
    """3. Every char a match (3000 per row: a group holds 192 000, many times the piece table), and matches alternating with one-char gaps:
    every 16-byte step is put together from eight or more pieces."""
    p, o = compiled("x")
    rows = [units("x" * 3000, np.uint8)] * (64 + 5)
    lists = oracle_all(o, rows[:1]) * len(rows)
    assert len(lists[0]) == 3000
    for repl in ("", "y", "yz"):
        check_replace(p, rows, lists, units(repl, np.uint8), np.uint8, what="every char a match")
    p, o = compiled("[0-9]+")
    for dtype in (np.uint8, np.uint16):
        rows = [units("1a" * 1500, dtype)] * (64 + 5)
        lists = oracle_all(o, rows[:1]) * len(rows)
        assert len(lists[0]) == 1500
        for repl in ("", "#", "<num>"):
            check_replace(p, rows, lists, units(repl, dtype), dtype, lead=2, trail=1, what="alternating")


@pytest.mark.gpu
@pytest.mark.parametrize("at", [0, 63, 64])
def test_long_gaps(at):
    """4. One 300 000-char row with matches only at its first 3 and last 3 chars, among 150 short rows: a gap of many sweeps."""
    p, o = compiled("[0-9]+")
    rng = np.random.default_rng(4 + at)
    short = layout_rows(rng, [ord(ch) for ch in "abc 0123"], [], n=150, max_len=60)
    long_row = rng.choice(units("abcxyz ", np.uint8), 300000)
    long_row[:3] = units("123", np.uint8)
    long_row[-3:] = units("456", np.uint8)
    rows = short[:at] + [long_row] + short[at:]
    lists = oracle_all(o, rows)
    assert lists[at] == [(0, 3), (299997, 300000)]
    for repl in ("#", "<number>"):  # shorter and longer than the match
        check_replace(p, rows, lists, units(repl, np.uint8), np.uint8, lead=7, trail=2, what=("long row at", at))
    check_replace(p, [r.astype(np.uint16) for r in rows], lists, units("#", np.uint16), np.uint16, lead=1, trail=0, what=("long row, 16 bit", at))


@pytest.mark.gpu
def test_insertion_and_termination():
    """5. An empty match is replaced once and ends its row: R in front of a row that starts with a non-matching char, and nothing else."""
    p, o = compiled("[a-c]*")
    rng = np.random.default_rng(5)
    rows = [np.concatenate([units("d", np.uint8), rng.choice(units("abcd", np.uint8), int(k))]) for k in rng.integers(0, 90, 200)]
    lists = oracle_all(o, rows)
    assert all(l == [(0, 0)] for l in lists)
    for repl in ("", "R", "<here>"):
        check_replace(p, rows, lists, units(repl, np.uint8), np.uint8, what="insertion at 0")
    p, o = compiled("a?")
    rows = [units("bbb", np.uint8)] * 130 + [units("abab", np.uint8), units("", np.uint8), units("aab", np.uint8)]
    lists = oracle_all(o, rows)
    assert lists[0] == [(0, 0)]
    want, _ = expected(rows[:1], lists[:1], units("RR", np.uint8), np.uint8)
    assert want.tobytes() == b"RRbbb"
    for dtype in (np.uint8, np.uint16):
        check_replace(p, [r.astype(dtype) for r in rows], lists, units("RR", dtype), dtype, what="a? on bbb")


@pytest.mark.gpu
def test_no_matches_at_all():
    """6. No match anywhere: the output is the input byte for byte (every block one piece), with start / end NULL."""
    import torch
    from needle_amd.pattern import Pattern
    for dtype in (np.uint8, np.uint16):
        rng = np.random.default_rng(6)
        rows = layout_rows(rng, [ord(ch) for ch in "abc xyz"], [], n=700, max_len=120, dtype=dtype)
        lists = [[] for _ in rows]
        for lead, out_start in ((5, 3), (0, 64), (11, 0)):
            check_splice(rows, lists, units("#", dtype), dtype, lead=lead, trail=7, out_start=out_start, no_lists=True, what="no matches")
        p, o = compiled("[0-9]+")
        data, offsets = device_packed(rows, dtype, lead=5, trail=7)
        out, out_off = p.replace_all_packed(data, offsets, "#")
        torch.cuda.synchronize()
        lo, hi = int(offsets[0]), int(offsets[-1])
        assert torch.equal(out, data[lo:hi]) and torch.equal(out_off, offsets - lo)


@pytest.mark.gpu
def test_stream_order():
    """7. The whole composition on a non-default stream with no synchronisation before the final check."""
    import torch
    p, o = compiled("[0-9]+")
    rng = np.random.default_rng(7)
    rows = layout_rows(rng, [ord(ch) for ch in "abcxyz 0123456789"], [], n=5000, max_len=200)
    lists = oracle_all(o, rows)
    repl = units("<n>", np.uint8)
    want, want_off = expected(rows, lists, repl, np.uint8)
    data, offsets = device_packed(rows, np.uint8, lead=5, trail=7, junk=[ord("7")])
    big, out, sent = guarded(want.size, 3, np.uint8)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    _, out_off = p.replace_all_packed(data, offsets, repl, stream=side.cuda_stream, out=out, out_start=3)
    first, ofirst = p.replace_first_packed(data, offsets, repl, stream=side.cuda_stream)
    side.synchronize()
    check_guarded(big, sent, want, want_off, out_off, 3, np.uint8, "side stream")
    wf, wf_off = expected(rows, [l[:1] for l in lists], repl, np.uint8)
    assert (first.cpu().numpy() == wf).all() and (ofirst.cpu().numpy() == wf_off).all()


@pytest.mark.gpu
@pytest.mark.parametrize("regex,cw,alphabet,plants,junk,ralpha", LAYOUT_PATTERNS)
def test_replace_first(layout_cases, regex, cw, alphabet, plants, junk, ralpha):
    """8. replace_first_packed against splice(row, oracle.find(row))."""
    import torch
    p, o, dtype, rows, _, jk = layout_cases(regex, cw, alphabet, plants, junk)
    found = [o.find(np.asarray(r)) for r in rows]
    lists = [[(s, e)] if f else [] for f, s, e in found]
    assert sum(len(l) for l in lists) > 100
    for k in (0, 3, 17):
        repl = np.resize(units(ralpha, dtype), k)
        want, want_off = expected(rows, lists, repl, dtype)
        data, offsets = device_packed(rows, dtype, lead=5, trail=7, junk=jk)
        big, out, sent = guarded(want.size, 3, dtype)
        _, out_off = p.replace_first_packed(data, offsets, repl, out=out, out_start=3)
        torch.cuda.synchronize()
        check_guarded(big, sent, want, want_off, out_off, 3, dtype, ("replace_first", regex, k))
    # numpy inputs: the same through an upload
    repl = np.resize(units(ralpha, dtype), 3)
    want, want_off = expected(rows, lists, repl, dtype)
    data, offsets = device_packed(rows, dtype, lead=2, trail=0, junk=jk)
    got, got_off = p.replace_first_packed(data.cpu().numpy().view(dtype), offsets.cpu().numpy(), repl)
    assert got.dtype == dtype and (got == want).all() and (got_off == want_off).all()


@pytest.mark.gpu
def test_splice_with_a_callers_list(layout_cases):
    """9. splice_packed with a list of the caller's own: every second match of the oracle's list dropped."""
    for case in (LAYOUT_PATTERNS[0], LAYOUT_PATTERNS[5], LAYOUT_PATTERNS[8]):
        regex, cw, alphabet, plants, junk, ralpha = case
        p, o, dtype, rows, lists, jk = layout_cases(regex, cw, alphabet, plants, junk)
        kept = [l[::2] for l in lists]
        assert sum(len(l) for l in kept) < sum(len(l) for l in lists)
        for k in (0, 2, 17):
            check_splice(rows, kept, np.resize(units(ralpha, dtype), k), dtype, lead=5, trail=7, out_start=3, what=("every second match", regex))
    # numpy inputs
    from needle_amd.pattern import Pattern
    regex, cw, alphabet, plants, junk, ralpha = LAYOUT_PATTERNS[0]
    p, o, dtype, rows, lists, jk = layout_cases(regex, cw, alphabet, plants, junk)
    kept = [l[::2] for l in lists]
    want, want_off = expected(rows, kept, units("#", dtype), dtype)
    off = np.zeros(len(rows) + 1, np.int64)
    off[1:] = np.cumsum([len(r) for r in rows])
    got, got_off = Pattern.splice_packed(np.concatenate(rows), off, *flatten(kept), "#")
    assert (got == want).all() and (got_off == want_off).all()


HOST_CHILD = r'''
import sys
sys.path.insert(0, "."); sys.path.insert(0, "tests")
import test_gpu_replace_all as T
T.host_entry_checks()
print("HOST-REPLACE-OK")
'''


def host_strings():
    rng = np.random.default_rng(10)
    words = ["call 555 0100 now", "", "x", "42", "no digits here", "a1b22c333", "7" * 300, "mixed 中文 12 λ 345", "trailing 9"]
    out = []
    for i in range(2000):
        k = int(rng.integers(0, 6))
        s = " ".join(words[int(j)] for j in rng.integers(0, len(words), k))
        out.append(s + ("z" * int(rng.integers(0, 400)) if i % 97 == 0 else ""))
    return out


def host_entry_checks():
    """replace_all_strings, the capacity protocol of needle_replace_all_packed_host and offsets that start above 0, against the oracle."""
    import ctypes
    from needle_amd import _lib
    from needle_amd.pattern import pack_strings
    p, o = compiled("[0-9]+")
    strings = host_strings()
    lists = [o.find_all(s, limit=1 << 30) for s in strings]
    for repl in ("#", "", "<number>"):
        want = [splice(s, l, repl) for s, l in zip(strings, lists)]
        assert p.replace_all_strings(strings, repl) == want, repl
    # the packed entry through numpy arrays, 8-bit rows, offsets[0] > 0 and junk around the rows
    rows = [np.frombuffer(s.encode("ascii", "replace"), np.uint8) for s in strings]
    lists8 = oracle_all(o, rows)
    want, want_off = expected(rows, lists8, units("<n>", np.uint8), np.uint8)
    data, offsets = device_packed(rows, np.uint8, lead=37, trail=9, junk=[ord("5")])
    hd, ho = data.cpu().numpy(), offsets.cpu().numpy()
    assert ho[0] >= 37
    got, got_off = p.replace_all_packed(hd, ho, "<n>")
    assert (got == want).all() and (got_off == want_off).all()
    # the capacity protocol on the raw entry
    L = _lib.lib()
    data16, off16 = pack_strings(strings)
    want16, want16_off = expected([units(s, np.uint16) for s in strings], lists, units("#", np.uint16), np.uint16)
    v = _lib.PackedView()
    v.data, v.char_width, v.n_rows, v.offsets = data16.ctypes.data, 2, len(strings), off16.ctypes.data
    r = units("#", np.uint16)
    out_off = np.full(len(strings) + 1, 99, np.uint64)
    total = ctypes.c_uint64(0)
    call = lambda text, cap: L.needle_replace_all_packed_host(p._h, ctypes.byref(v), r.ctypes.data, r.size, out_off.ctypes.data,
                                                              text.ctypes.data if text is not None else None, cap, ctypes.byref(total))
    assert call(None, 0) == 0 and total.value == want16.size and (out_off.astype(np.int64) == want16_off).all()   # sizes only
    small = np.full(want16.size // 2 + 16, 0xA5A5, np.uint16)
    out_off[:] = 99
    assert call(small[:-16], small.size - 16) == 0 and total.value == want16.size and (out_off.astype(np.int64) == want16_off).all()
    assert (small[-16:] == 0xA5A5).all()                                                                          # too small: nothing past capacity
    exact = np.full(want16.size + 16, 0xA5A5, np.uint16)
    assert call(exact[:-16], want16.size) == 0 and total.value == want16.size
    assert (exact[:-16] == want16).all() and (exact[-16:] == 0xA5A5).all()


@pytest.mark.gpu
def test_host_entry():
    """10. The host entry: 2000 mixed-length strings in one chunk (here) and in several (a child process: NEEDLE_HOST_CHUNK_BYTES and
    NEEDLE_HOST_RESULT_BYTES are read once per process), the capacity protocol, offsets that start above 0."""
    host_entry_checks()
    env = dict(os.environ, NEEDLE_HOST_CHUNK_BYTES="20000", NEEDLE_HOST_RESULT_BYTES="4096")
    r = subprocess.run([sys.executable, "-c", HOST_CHILD], env=env, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert "HOST-REPLACE-OK" in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]
