"""Replace each match by the replacement its choice names, or keep it, on the device (needle_replace_each_lengths_packed_dev /
needle_replace_each_fill_packed_dev / needle_set_replace_each_packed_host; Pattern.splice_each_packed, PatternSet.replace_each_packed /
replace_each_strings / replace_each_bytes): bit-exact against splice_each (tests/test_replace_each_abi.py) of the oracle's lists, no
tolerances.  Every device run writes into a buffer with 64 sentinel code units in front of out_offsets[0] and 64 behind out_offsets[n];
they must come back untouched."""
import os
import random
import subprocess
import sys

import numpy as np
import pytest

from test_gpu_configs import compiled
from test_gpu_find_all_packed import oracle_all
from test_gpu_packed_dev import device_packed, layout_rows
from test_gpu_replace_all import LAYOUT_PATTERNS, check_guarded, flatten, guarded, host_strings, units
from test_replace_each_abi import splice_each

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INT32_MIN, INT32_MAX = -2 ** 31, 2 ** 31 - 1
PATTERNS = [LAYOUT_PATTERNS[i] for i in (0, 4, 5, 8)]  # [0-9]+ at cw 1, international|inter|nation at cw 1 and 2, Greek / Cyrillic / CJK at cw 2
assert [(p[0], p[1]) for p in PATTERNS] == [("[0-9]+", 1), ("international|inter|nation", 1), ("international|inter|nation", 2),
                                            ("[α-ω]{2}[α-ω]*|ЖЗ+|中文", 2)]


@pytest.fixture(scope="module", autouse=True)
def built():
    from needle_amd import build
    build.build()
    from oracle import walker
    walker.build()


def draw_choices(rng, lists, n_repl, kept=0.3):
    """Per row a choice per match: a table entry, or one of the values that keep the match -- for every fourth match of the batch, and
    with probability `kept` for the others, so that at least a quarter is kept."""
    keep = [INT32_MIN, -1, n_repl, INT32_MAX]
    out, k = [], 0
    for l in lists:
        out.append([keep[int(rng.integers(4))] if (k + i) % 4 == 0 or rng.random() < kept else int(rng.integers(n_repl)) for i in range(len(l))])
        k += len(l)
    flat = [c for x in out for c in x]
    assert sum(1 for c in flat if not 0 <= c < n_repl) * 4 >= len(flat), "at least a quarter kept"
    return out


def tables(ralpha, dtype):
    """The three tables of the layout tests: short entries with an empty one, 256 one-unit entries, one entry of 4096 units between two empty ones."""
    a = units(ralpha, dtype)
    return [[np.resize(a, 0), np.resize(a, 1), np.resize(a[1:], 3), np.resize(a, 17)],
            [np.array([0x4E00 + i if dtype == np.uint16 else 33 + i % 94], dtype) for i in range(256)],
            [np.resize(a, 0), np.resize(a, 4096), np.resize(a, 0)]]


def expected_each(rows, lists, choices, repls, dtype):
    out = [splice_each(np.asarray(r, dtype), l, c, repls) for r, l, c in zip(rows, lists, choices)]
    off = np.zeros(len(rows) + 1, np.int64)
    off[1:] = np.cumsum([len(x) for x in out])
    return (np.concatenate(out) if out else np.zeros(0, dtype)).astype(dtype), off


def device_list(lists, choices):
    import torch
    moff, st, en = flatten(lists)
    ch = np.array([c for x in choices for c in x], np.int64).astype(np.int32)
    return tuple(torch.from_numpy(x).to("cuda") for x in (moff, st, en, ch))


def check_each(rows, lists, choices, repls, dtype, lead=5, trail=7, junk=None, out_start=3, lowest_bit=False, want=None, stream=None, what=""):
    """splice_each_packed of the rows and the list into a guarded buffer against the reference (or `want` = (text, offsets from 0))."""
    import torch
    from needle_amd.pattern import Pattern
    text, off = expected_each(rows, lists, choices, repls, dtype) if want is None else want
    data, offsets = device_packed(rows, dtype, lead=lead, trail=trail, junk=junk)
    moff, st, en, ch = device_list(lists, choices)
    big, out, sent = guarded(text.size, out_start, dtype)
    got, out_off = Pattern.splice_each_packed(data, offsets, moff, st, en, ch, repls, stream=stream, out=out, out_start=out_start, lowest_bit=lowest_bit)
    assert got.data_ptr() == out.data_ptr()
    torch.cuda.synchronize()
    check_guarded(big, sent, text, off, out_off, out_start, dtype, (what, "entries", len(repls), "lead", lead, "out_start", out_start))
    return data, offsets, out_off


_layout = {}


def layout_case(regex, cw, alphabet, plants, junk):
    """(pattern, oracle, dtype, rows, the oracle's lists, junk) per pattern: the recipe of test_gpu_replace_all, made once."""
    key = (regex, cw)
    if key not in _layout:
        p, o = compiled(regex)
        dtype = np.uint8 if cw == 1 else np.uint16
        rng = np.random.default_rng(17 + len(regex) + cw)
        rows = layout_rows(rng, [ord(ch) for ch in alphabet], plants, n=700, max_len=120, dtype=dtype)
        _layout[key] = (p, o, dtype, rows, oracle_all(o, rows), [ord(ch) for ch in junk])
    return _layout[key]


@pytest.mark.gpu
@pytest.mark.parametrize("regex,cw,alphabet,plants,junk,ralpha", PATTERNS)
def test_layouts(regex, cw, alphabet, plants, junk, ralpha):
    """1. Patterns x tables x char widths x layouts x batch sizes, and only empty rows."""
    p, o, dtype, rows, lists, jk = layout_case(regex, cw, alphabet, plants, junk)
    assert sum(len(l) for l in lists) > 100
    for t, repls in enumerate(tables(ralpha, dtype)):
        rng = np.random.default_rng(100 + t)
        choices = draw_choices(rng, lists, len(repls))
        want = expected_each(rows, lists, choices, repls, dtype)
        check_each(rows, lists, choices, repls, dtype, lead=5, trail=7, junk=jk, out_start=3, want=want, what="lead 5 trail 7")
        check_each(rows, lists, choices, repls, dtype, lead=0, trail=0, junk=jk, out_start=64, want=want, what="offsets[0] = 0, out_offsets[0] = 64")
        check_each(rows, lists, choices, repls, dtype, lead=133, trail=0, junk=jk, out_start=3, want=want, what="offsets[0] > 0")
        for n in (1, 63, 65, 130):
            check_each(rows[48:48 + n], lists[48:48 + n], choices[48:48 + n], repls, dtype, lead=3, trail=5, junk=jk, what="n_rows %d" % n)
        empty = [np.zeros(0, dtype)] * 70
        el = oracle_all(o, empty)
        check_each(empty, el, draw_choices(rng, el, len(repls)), repls, dtype, lead=9, trail=9, junk=jk, what="70 empty rows")


@pytest.mark.gpu
@pytest.mark.parametrize("regex,cw,alphabet,plants,junk,ralpha", PATTERNS)
def test_one_entry_chosen_everywhere_is_replace_all(regex, cw, alphabet, plants, junk, ralpha):
    """2. n_repl = 1 and every choice 0: the bytes and the offsets Pattern.splice_packed -- the plain kernels -- gives for the same list."""
    import torch
    from needle_amd.pattern import Pattern
    p, o, dtype, rows, lists, jk = layout_case(regex, cw, alphabet, plants, junk)
    data, offsets = device_packed(rows, dtype, lead=5, trail=7, junk=jk)
    moff, st, en, ch = device_list(lists, [[0] * len(l) for l in lists])
    for k in (0, 3, 4096):
        repl = np.resize(units(ralpha, dtype), k)
        plain, plain_off = Pattern.splice_packed(data, offsets, moff, st, en, repl)
        torch.cuda.synchronize()
        want, want_off = plain.cpu().numpy().view(dtype), plain_off.cpu().numpy()
        for form in (False, True):  # (as masks: bit 0 alone)
            big, out, sent = guarded(want.size, 3, dtype)
            _, out_off = Pattern.splice_each_packed(data, offsets, moff, st, en, ch + 1 if form else ch, [repl], out=out, out_start=3, lowest_bit=form)
            torch.cuda.synchronize()
            check_guarded(big, sent, want, want_off, out_off, 3, dtype, ("against splice_packed", regex, k, form))


@pytest.mark.gpu
@pytest.mark.parametrize("regex,cw,alphabet,plants,junk,ralpha", PATTERNS)
def test_all_kept(regex, cw, alphabet, plants, junk, ralpha):
    """3. Every match kept: the output is the input span byte for byte, out_offsets = offsets - offsets[0] + out_start."""
    import torch
    p, o, dtype, rows, lists, jk = layout_case(regex, cw, alphabet, plants, junk)
    rng = np.random.default_rng(3)
    text = np.concatenate(rows).astype(dtype)
    off = np.zeros(len(rows) + 1, np.int64)
    off[1:] = np.cumsum([len(r) for r in rows])
    for repls in tables(ralpha, dtype):
        choices = draw_choices(rng, lists, len(repls), kept=1.0)
        for lead, out_start in ((5, 3), (0, 64), (133, 0)):
            data, offsets, out_off = check_each(rows, lists, choices, repls, dtype, lead=lead, trail=0 if lead != 5 else 7, junk=jk, out_start=out_start,
                                                want=(text, off), what="all kept")
            assert torch.equal(out_off, offsets - offsets[0] + out_start)


@pytest.mark.gpu
@pytest.mark.parametrize("row", ["x", "xy"])
def test_shared_edges(row):
    """4. 200 one-match rows, replaced by a longer, an empty and a shorter-or-equal entry or kept in turn: the groups' output spans meet
    at every alignment inside a dword and inside a 16-byte block, on the input side (lead) and on the output side (out_offsets[0])."""
    rows = [units(row, np.uint8)] * 200
    lists = [[(0, 1)]] * 200
    repls = [units(s, np.uint8) for s in ("abc", "", "ab")]
    choices = [[r % 4 - 1] for r in range(200)]
    want = expected_each(rows, lists, choices, repls, np.uint8)
    for lead in range(16):
        trail = (-(lead + 200 * len(row))) % 4  # (so that device_packed keeps the lead as it is)
        for out_start in range(16):
            check_each(rows, lists, choices, repls, np.uint8, lead=lead, trail=trail, out_start=out_start, want=want, what=("edges", row))


@pytest.mark.gpu
def test_more_matches_than_a_chunk():
    """5. Every char a match (3000 per row: a group holds 192 000, many times the piece table) with entries of 0 .. 3 bytes and kept
    matches in a cycle of five: the entries start at odd bytes of the table and every 16-byte step is put together from eight or more
    pieces of differing lengths; and matches alternating with one-char gaps at both widths."""
    p, o = compiled("x")
    rows = [units("x" * 3000, np.uint8)] * (64 + 5)
    lists = oracle_all(o, rows[:1]) * len(rows)
    assert len(lists[0]) == 3000
    repls = [units(s, np.uint8) for s in ("", "y", "yz", "pqr")]
    for cycle in ([1, 2, 3, -1, 0], [3, INT32_MAX, 1, 2, 3, 0, 2]):
        choices = [[cycle[(i + r) % len(cycle)] for i in range(3000)] for r in range(len(rows))]
        check_each(rows, lists, choices, repls, np.uint8, what="every char a match")
    p, o = compiled("[0-9]+")
    for dtype in (np.uint8, np.uint16):
        rows = [units("1a" * 1500, dtype)] * (64 + 5)
        lists = oracle_all(o, rows[:1]) * len(rows)
        assert len(lists[0]) == 1500
        repls = [units(s, dtype) for s in ("", "#", "<num>", "ab")]
        choices = [[(i + 3 * r) % 6 - 1 for i in range(1500)] for r in range(len(rows))]  # (-1 and 4: kept)
        check_each(rows, lists, choices, repls, dtype, lead=2, trail=1, what="alternating")


@pytest.mark.gpu
@pytest.mark.parametrize("at", [0, 63, 64])
def test_long_gaps(at):
    """6. One 300 000-char row with matches only at its first 3 and last 3 chars, among 150 short rows: a gap of many sweeps; the first
    match replaced by a longer entry, the last by a shorter one."""
    p, o = compiled("[0-9]+")
    rng = np.random.default_rng(4 + at)
    short = layout_rows(rng, [ord(ch) for ch in "abc 0123"], [], n=150, max_len=60)
    long_row = rng.choice(units("abcxyz ", np.uint8), 300000)
    long_row[:3] = units("123", np.uint8)
    long_row[-3:] = units("456", np.uint8)
    rows = short[:at] + [long_row] + short[at:]
    lists = oracle_all(o, rows)
    assert lists[at] == [(0, 3), (299997, 300000)]
    names = ("#", "<number>", "", "seven77")
    choices = draw_choices(rng, lists, len(names))
    choices[at] = [1, 0]
    check_each(rows, lists, choices, [units(s, np.uint8) for s in names], np.uint8, lead=7, trail=2, what=("long row at", at))
    check_each([r.astype(np.uint16) for r in rows], lists, choices, [units(s, np.uint16) for s in names], np.uint16, lead=1, trail=0,
               what=("long row, 16 bit", at))


@pytest.mark.gpu
def test_mask_form():
    """7. Choices as masks: 0 keeps, the lowest set bit names the entry (1 << 31 alone with 32 entries: entry 31), a lowest bit at or
    above n_repl keeps (1 << 5 with 5 entries); the result is the index form's with first_member's indices, and the reference's."""
    from needle_amd.pattern import PatternSet
    regex, cw, alphabet, plants, junk, ralpha = PATTERNS[0]
    p, o, dtype, rows, lists, jk = layout_case(regex, cw, alphabet, plants, junk)
    rng = np.random.default_rng(7)
    fixed = [0, 1 << 31, 1 << 5, 0b1010, 0xFFFFFFFF, (1 << 31) | (1 << 30), 0b110000]
    for n_repl in (32, 5):
        repls = [units("<%d>" % i, dtype)[:1 + i % 4] for i in range(n_repl)]
        masks = [[fixed[int(rng.integers(len(fixed)))] if rng.random() < 0.7 else int(rng.integers(1, 2 ** 32)) for _ in l] for l in lists]
        index = [PatternSet.first_member(np.array(m, np.uint32)).tolist() for m in masks]
        assert PatternSet.first_member(np.array(fixed[:4], np.uint32)).tolist() == [-1, 31, 5, 1]
        want = expected_each(rows, lists, index, repls, dtype)
        as_int32 = [np.array(m, np.uint32).view(np.int32).tolist() for m in masks]
        check_each(rows, lists, as_int32, repls, dtype, junk=jk, lowest_bit=True, want=want, what=("masks", n_repl))
        check_each(rows, lists, index, repls, dtype, junk=jk, want=want, what=("first_member's indices", n_repl))
    flat = [c for x in index for c in x]
    assert flat.count(-1) > 10 and sum(1 for c in flat if c >= 5) > 10 and flat.count(1) > 10  # (n_repl 5: mask 0, bits at or above 5, entry 1)


SET_NAMES = ["logs8", "nullable4", "u16b", "count260ci"]  # (count260ci: per-lane find-all, tags from a 16-bit table with flags, the splice)
_sets = {}


def set_case(name):
    """(set, its union pattern, dtype, rows, the oracle's union list per row, per match the lowest member of the reference masks, the
    table: one entry per member, an empty one among them) -- once per set."""
    if name not in _sets:
        from needle_amd.pattern import PatternSet
        from pattern_set_cases import compile_set
        from set_spans_cases import reference_span_masks, union_spans
        ps, oracles, dtype = compile_set(name)
        rows, spans = union_spans(name)
        first = PatternSet.first_member(reference_span_masks(oracles, rows, spans))
        off = spans[0]
        lists = [list(zip(spans[1][off[r]:off[r + 1]].tolist(), spans[2][off[r]:off[r + 1]].tolist())) for r in range(len(rows))]
        choices = [first[off[r]:off[r + 1]].tolist() for r in range(len(rows))]
        repls = ["" if i == 2 else "<%s%d>" % ("规" if dtype == np.uint16 else "r", i) * (1 + i % 3) for i in range(ps.n_patterns)]
        _sets[name] = (ps, ps.union_pattern(), oracles, dtype, rows, lists, choices, repls)
    return _sets[name]


@pytest.mark.gpu
@pytest.mark.parametrize("name", SET_NAMES)
def test_sets_end_to_end(name):
    """8. PatternSet.replace_each_packed on device tensors and replace_each_strings against splice_each of the oracle's union list with
    the lowest member of the reference masks."""
    import torch
    from pattern_set_cases import units as set_units
    from test_gpu_pattern_set import JUNK
    ps, u, oracles, dtype, rows, lists, choices, repls = set_case(name)
    flat = [c for x in choices for c in x]
    assert len(flat) > 90 and len(set(flat)) >= 3, (len(flat), sorted(set(flat)))
    table = [units(s, dtype) for s in repls]
    want, want_off = expected_each(rows, lists, choices, table, dtype)
    data, offsets = device_packed(rows, dtype, lead=5, trail=7, junk=set_units(JUNK[name], dtype))
    big, out, sent = guarded(want.size, 3, dtype)
    got, out_off = ps.replace_each_packed(u, data, offsets, repls, out=out, out_start=3)
    assert got.data_ptr() == out.data_ptr()
    torch.cuda.synchronize()
    check_guarded(big, sent, want, want_off, out_off, 3, dtype, ("set", name))
    some = [r for r in range(len(rows)) if r not in (70, 71)]  # (not the two long rows)
    strings = ["".join(chr(int(c)) for c in rows[r]) for r in some]
    assert len(strings) > 200
    assert ps.replace_each_strings(strings, repls) == [splice_each(s, lists[r], choices[r], repls) for s, r in zip(strings, some)]
    assert ps.replace_each_strings(strings[:40], repls, pattern=u) == [splice_each(s, lists[r], choices[r], repls) for s, r in zip(strings[:40], some)]


@pytest.mark.gpu
def test_stream_order():
    """9. The whole composition -- find-all, tags, lengths, cumsum, fill -- on a side stream with no synchronisation before the final check."""
    import torch
    from pattern_set_cases import units as set_units
    from test_gpu_pattern_set import JUNK
    ps, u, oracles, dtype, rows, lists, choices, repls = set_case("logs8")
    want, want_off = expected_each(rows, lists, choices, [units(s, dtype) for s in repls], dtype)
    data, offsets = device_packed(rows, dtype, lead=5, trail=7, junk=set_units(JUNK["logs8"], dtype))
    big, out, sent = guarded(want.size, 3, dtype)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    _, out_off = ps.replace_each_packed(u, data, offsets, repls, stream=side.cuda_stream, out=out, out_start=3)
    side.synchronize()
    check_guarded(big, sent, want, want_off, out_off, 3, dtype, "side stream")


HOST_CHILD = r'''
import sys
sys.path.insert(0, "."); sys.path.insert(0, "tests")
from oracle import walker; walker.build()
import test_gpu_replace_each as T
T.host_entry_checks()
print("HOST-REPLACE-EACH-OK")
'''
HOST_MEMBERS = ["[0-9][0-9]+", "call|now|here", "中文|λ", "z+"]  # (a single digit and the other words match no member: kept)
HOST_PATTERN = "[0-9]+|[a-z]+|中文|λ"
HOST_REPLS = ["<n>", "", "汉字 and more", "Z"]


def host_reference(p_oracle, member_oracles, rows):
    lists = oracle_all(p_oracle, rows)
    choices = [[next((i for i, m in enumerate(member_oracles) if m.matches(np.ascontiguousarray(r[s:e]))), -1) for s, e in l] for r, l in zip(rows, lists)]
    return lists, choices


def host_entry_checks():
    """replace_each_strings with a pattern of the caller's, the packed entry through numpy arrays with offsets[0] > 0, and the capacity
    protocol of needle_set_replace_each_packed_host, against the oracle."""
    import ctypes
    from needle_amd import _lib
    from needle_amd.pattern import DFACompiler, Pattern, PatternSet, pack_strings
    from test_compile_matches_txt import oracle_for
    p, o = compiled(HOST_PATTERN)
    ps = PatternSet([DFACompiler.compile(m) for m in HOST_MEMBERS])
    members = [oracle_for(m, 0)[0] for m in HOST_MEMBERS]
    strings = host_strings()
    rows16 = [units(s, np.uint16) for s in strings]
    lists, choices = host_reference(o, members, rows16)
    flat = [c for x in choices for c in x]
    assert all(flat.count(c) > 3 for c in (-1, 0, 1, 2, 3)), [flat.count(c) for c in (-1, 0, 1, 2, 3)]
    want = [splice_each(s, l, c, HOST_REPLS) for s, l, c in zip(strings, lists, choices)]
    assert ps.replace_each_strings(strings, HOST_REPLS, pattern=p) == want
    # the packed entry through numpy arrays, 8-bit rows, offsets[0] > 0 and junk around the rows
    rows8 = [np.frombuffer(s.encode("ascii", "replace"), np.uint8) for s in strings]
    lists8, choices8 = host_reference(o, members, rows8)
    repls8 = [units(s, np.uint8) for s in ("<n>", "", "two", "Z")]
    want8, want8_off = expected_each(rows8, lists8, choices8, repls8, np.uint8)
    data, offsets = device_packed(rows8, np.uint8, lead=37, trail=9, junk=[ord("5")])
    hd, ho = data.cpu().numpy(), offsets.cpu().numpy()
    assert ho[0] >= 37
    got, got_off = ps.replace_each_packed(p, hd, ho, repls8)
    assert (got == want8).all() and (got_off == want8_off).all()
    # the capacity protocol on the raw entry
    L = _lib.lib()
    data16, off16 = pack_strings(strings)
    want16, want16_off = expected_each(rows16, lists, choices, [units(s, np.uint16) for s in HOST_REPLS], np.uint16)
    v = _lib.PackedView()
    v.data, v.char_width, v.n_rows, v.offsets = data16.ctypes.data, 2, len(strings), off16.ctypes.data
    r, roff = Pattern._repl_table(HOST_REPLS, 2)
    out_off = np.full(len(strings) + 1, 99, np.uint64)
    total = ctypes.c_uint64(0)
    call = lambda text, cap: L.needle_set_replace_each_packed_host(ps._h, p._h, ctypes.byref(v), r.ctypes.data, roff.ctypes.data, roff.size - 1,
                                                                   out_off.ctypes.data, text.ctypes.data if text is not None else None, cap,
                                                                   ctypes.byref(total))
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
    assert "HOST-REPLACE-EACH-OK" in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]


@pytest.mark.gpu
def test_utf8_rows():
    """11. replace_each_bytes on UTF-8 rows of ASCII, 2- / 3- / 4-byte sequences and ill-formed bytes: the splice of the ORIGINAL bytes
    at the byte spans find_all_bytes of the union gives, each span tagged by the members' oracles on its decoded text; a match next to a
    surrogate pair; ill-formed bytes outside replaced matches untouched."""
    from needle_amd.pattern import DFACompiler, PatternSet
    from test_compile_matches_txt import oracle_for
    from utf8_cases import _ILL, mixed_bytes
    members = ["[0-9]+", "ERROR|FATAL", "[а-я]+", "中文"]
    ps = PatternSet([DFACompiler.compile(m) for m in members])
    oracles = [oracle_for(m, 0)[0] for m in members]
    repls = [b"<n>", b"E", "<слово>".encode("utf-8"), b""]
    rng = random.Random(11)
    rows = [mixed_bytes(rng.randrange(0, 60), rng, words=("ERROR", "42", "中文", "FATAL7")) for _ in range(300)]
    rows += ["\U0001F600ERROR\U0001F601".encode("utf-8"), "x\U0001F60042\U0001F600да".encode("utf-8"), b"", b"\xF0\x9F\x98ERROR\x80",
             b"".join(_ILL), b"\xFF12\xC0\xAF"]
    u = ps.union_pattern()
    spans = u.find_all_bytes(rows)
    assert spans[300] == [(4, 9)] and spans[301] == [(5, 7), (11, 15)] and spans[303] == [(3, 8)] and spans[304] == [] and spans[305] == [(1, 3)]
    assert sum(len(s) for s in spans) > 100

    def member(b):
        t = units(b.decode("utf-8"), np.uint16)  # (the members match well-formed text only)
        return next((i for i, o in enumerate(oracles) if o.matches(t)), -1)
    choices = [[member(row[s:e]) for s, e in l] for row, l in zip(rows, spans)]
    flat = [c for x in choices for c in x]
    assert all(flat.count(c) > 3 for c in range(4)) and -1 not in flat  # (every union match is some member's)
    want = [splice_each(row, l, c, repls) for row, l, c in zip(rows, spans, choices)]
    assert want[300] == "\U0001F600E\U0001F601".encode("utf-8") and want[303] == b"\xF0\x9F\x98E\x80" and want[305] == b"\xFF<n>\xC0\xAF"
    assert ps.replace_each_bytes(rows, repls) == want
    # a pattern of the caller's whose matches no member matches whole: every byte comes back, ill-formed ones included
    assert ps.replace_each_bytes(rows, repls, pattern=DFACompiler.compile("[A-Z]|[0-9]+x")) == rows
