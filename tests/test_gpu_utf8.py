"""UTF-8 packed rows on the device (needle_utf16_lengths_from_utf8_packed_dev / needle_utf16_from_utf8_packed_dev /
needle_utf8_positions_packed_dev, the needle_*_utf8_packed_host entries and Pattern's *_utf8_packed / *_bytes methods): bit-exact against
the rule restated in utf8_cases.py (pinned to CPython's decoder by test_utf8_abi.py), no tolerances.  The input lies between a leading
sentinel that ends in E2 82 and a trailing one that starts with AC -- neither may be read as part of the batch -- and every output
between at least 64 sentinel entries that must come back untouched."""
import os
import random
import subprocess
import sys

import numpy as np
import pytest

import utf8_cases as U
from test_gpu_configs import compiled
from test_replace_abi import splice

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 64


def guarded(n, dtype, sent, front=0):
    """A device tensor of sentinels: GUARD + front entries, room for n, GUARD more (a multiple of 4 bytes) -> (whole, the view behind GUARD)."""
    import torch
    size = GUARD + front + n + GUARD
    size += (-size) % 4
    big = torch.from_numpy(np.full(size, sent, dtype)).to("cuda")
    return big, big[GUARD:]


def check_transcode(rows, want=None, shift=0, out_start=0, what=""):
    """lengths, both bitmaps and the filled units of the rows against the rule; sentinels around the input and the output."""
    import torch
    from needle_amd.pattern import Pattern
    want = U.Expected(rows) if want is None else want
    data, offsets, host = U.device_utf8(rows, shift=shift)
    total = int(want.lengths.sum())
    big, out = guarded(total, np.int16, -23131, front=out_start)  # 0xA5A5
    units, uoff, na, mal = Pattern.utf16_from_utf8_packed(data, offsets, out=out, out_start=out_start)
    torch.cuda.synchronize()
    assert (data.cpu().numpy() == host).all(), ("input", what)
    assert (uoff.cpu().numpy() == want.unit_offsets(out_start)).all(), ("unit offsets", what)
    assert (na.cpu().numpy().view(np.uint64) == U.bitmap(want.non_ascii)).all(), ("non-ASCII bitmap", what)
    assert (mal.cpu().numpy().view(np.uint64) == U.bitmap(want.malformed)).all(), ("malformed bitmap", what)
    got = big.cpu().numpy().view(np.uint16)
    a, b = GUARD + out_start, GUARD + out_start + total
    assert (got[:a] == 0xA5A5).all() and (got[b:] == 0xA5A5).all(), ("sentinels", what, np.nonzero(got[:a] != 0xA5A5)[0][:8], np.nonzero(got[b:] != 0xA5A5)[0][:8])
    bad = np.nonzero(got[a:b] != want.units)[0]
    assert bad.size == 0, ("units", what, bad[:8], got[a:b][bad[:8]], want.units[bad[:8]])
    return data, offsets, want


def check_positions(data, offsets, lst, what=""):
    """utf8_positions_packed on a list and its answers (Expected.position_list); only [list_off[0], list_off[n]) is written."""
    import torch
    from needle_amd.pattern import Pattern
    off, pos, ans = lst
    first, m = int(off[0]), pos.size
    big, out = guarded(m, np.int32, -77)
    dev = lambda x: torch.from_numpy(x).to("cuda")
    Pattern.utf8_positions_packed(data, offsets, dev(off), dev(pos), out=out)
    torch.cuda.synchronize()
    got = big.cpu().numpy()
    assert (got[:GUARD + first] == -77).all() and (got[GUARD + m:] == -77).all(), ("entries outside the list", what)
    bad = np.nonzero(got[GUARD + first:GUARD + m] != ans[first:])[0]
    assert bad.size == 0, ("byte positions", what, bad[:8], got[GUARD + first:GUARD + m][bad[:8]], ans[first:][bad[:8]], pos[first:][bad[:8]])


@pytest.fixture(scope="module")
def exhaustive():
    rows = U.alphabet_rows()
    assert len(rows) == 406900
    return U.Expected(rows)


PADS = {0: [], 1: [b"\xC3"], 2: [b"\xE2\x82", b"a\xF0\x9F"], 3: [b"\xF0\x9F\x98\x80", b"\xE2\x82\xACab", b"\x80"]}


@pytest.mark.parametrize("pads", [0, 1, 2, 3])
def test_exhaustive_rows_of_one_to_four_alphabet_bytes(exhaustive, pads):
    """1. Every row of 1 to 4 alphabet bytes back to back in ONE batch -- neighbouring rows complete each other's sequences in every
    combination -- as it is and behind 1, 2 and 3 pad rows (1, 5 and 10 bytes: every sequence meets every block, step and group boundary)."""
    want = U.Expected.join(U.Expected(PADS[pads]), exhaustive) if pads else exhaustive
    data, offsets, _ = check_transcode(want.rows, want, what=("pads", pads))
    if pads in (0, 3):  # 4. every position 0 .. U of every row, U + 5 (clamped) and -1 (passed through), in one list
        check_positions(data, offsets, want.position_list(extra=lambda u: (u + 5, -1), first=3), what=("exhaustive", pads))
    if pads == 0:
        check_positions(data, offsets, want.position_list(extra=lambda u: (u + 5, -1), order="reversed"), what="exhaustive, reversed")
        check_positions(data, offsets, want.position_list(extra=lambda u: (u + 5, -1), order=random.Random(7)), what="exhaustive, shuffled")


def test_edges():
    """2. Row counts around the group size, empty rows at both ends and in runs of a group and more, a batch of empty rows only, spans
    shorter than a block at each of the 16 alignments, an output that starts at an odd unit."""
    rng = random.Random(3)
    for n in (1, 63, 64, 65, 130):
        rows = [U.mixed_bytes(rng.randrange(0, 12), rng, weights=(40, 20, 20, 15, 5)) for _ in range(n)]
        for out_start in (0, 1, 3):
            data, offsets, want = check_transcode(rows, out_start=out_start, what=("n_rows", n, out_start))
        check_positions(data, offsets, want.position_list(extra=lambda u: (u + 5, -1)), what=("n_rows", n))
    body = [U.mixed_bytes(rng.randrange(1, 30), rng, weights=(40, 20, 20, 15, 5)) for _ in range(70)]
    for rows in ([b""] + body + [b""], [b""] * 64 + body + [b""] * 130, body[:10] + [b""] * 200 + body[10:], [b""] * 64 + body[:3], [b""] * 1, [b""] * 64, [b""] * 200):
        data, offsets, want = check_transcode(rows, what=("empty rows", len(rows)))
        check_positions(data, offsets, want.position_list(extra=(0, 7, -1)), what=("empty rows", len(rows)))
    from needle_amd.pattern import Pattern
    data, offsets, _ = U.device_utf8([b"", b"", b""])  # a result of no units, into the method's own allocation
    units, uoff, na, mal = Pattern.utf16_from_utf8_packed(data, offsets)
    assert units.numel() == 0 and uoff.tolist() == [0, 0, 0, 0] and na.tolist() == [0] and mal.tolist() == [0]
    for shift in range(16):
        for rows in ([b"\xE2\x82\xAC\xF0\x9F\x98\x80\xC3"], [b"\xAC", b"", b"\xF0\x9F\x98", b"\x80\xE2\x82", b"\xACz"]):
            check_transcode(rows, shift=shift, out_start=shift % 4, what=("short span", shift))


@pytest.fixture(scope="module")
def long_batch():
    rng = random.Random(5)
    small = [U.mixed_bytes(rng.randrange(0, 11), rng) for _ in range(150)]
    assert max(len(r) for r in small) <= 40
    return U.long_row(70001, seed=6), small


@pytest.mark.parametrize("where", ["middle", "first", "last"])
def test_long_row(long_batch, where):
    """3. One row of 70 001 bytes -- longer than 65 535 and than any step of a wave -- among short rows: in the middle of its 64-row
    group, first and last in it.  4. Every position of every row in file order; reversed and shuffled lists with 64 sampled positions of
    the long row (every decreasing entry restarts the row's sweep: the whole row reversed would be 38 000 sweeps by one lane)."""
    long, small = long_batch
    at = {"middle": 70, "first": 64, "last": 127}[where]
    rows = small[:at] + [long] + small[at:]
    data, offsets, want = check_transcode(rows, what=("long row", where))
    assert want.lengths[at] > 30000 and want.malformed[at]
    check_positions(data, offsets, want.position_list(extra=lambda u: (u + 5, -1), first=2), what=("long row", where))
    if where == "middle":
        check_positions(data, offsets, want.position_list(extra=lambda u: (u + 5, -1), order="reversed", cap=64), what="reversed")
        check_positions(data, offsets, want.position_list(extra=lambda u: (u + 5, -1), order=random.Random(7), cap=64), what="shuffled")
        check_positions(data, offsets, want.position_list(rows=[0, 3, at, 100, len(rows) - 1]), what="entries in some rows")
        check_positions(data, offsets, want.position_list(rows=[]), what="an empty list, NULL arrays")


def test_three_byte_sequences_across_every_step_boundary():
    """3. Rows of 3-byte sequences five steps long, behind 0, 1 and 2 ASCII bytes and at every alignment of the row's first byte: a
    sequence lies across every step boundary with one byte and with two bytes in front of it."""
    from needle_amd import _lib
    window = _lib.lib().needle_utf8_window_bytes()
    for lead in (0, 1, 2):
        row = b"x" * lead + "€".encode() * (5 * window // 3)
        for shift in (0, 1, 2, 7, 15):
            data, offsets, want = check_transcode([b"ab", row, b"\xAC"], shift=shift, what=("steps", lead, shift))
        assert want.lengths[1] == lead + 5 * window // 3 and not want.malformed[1]
        check_positions(data, offsets, want.position_list(), what=("steps", lead))


# ---- 5. end to end
CI_UCASE = 0x02 | 0x40
PATTERNS = [("[0-9]+", 0), ("Sherlock", 0), ("[Ss]herlock", 0), ("Sherlock|Street", 0), ("ε", 0), ("ε|λ", 0), ("a.c", 0), ("(ab|a|bcdef|g)+", 0),
            ("[а-я]+", 0), (".", 0), ("[^a]", 0), ("привет|sherlock", CI_UCASE)]
WORDS = ["Sherlock", "sherlock", "Street", "ε", "λ", "abc", "a😀c", "aяc", "abcdefg", "привет", "ПРИВЕТ", "SHERLOCK", "2024", "7"]


@pytest.fixture(scope="module")
def e2e_rows():
    rng = random.Random(17)
    mixed = [U.mixed_bytes(rng.randrange(0, 24), rng, words=WORDS) for _ in range(64 * 300)]
    ascii_rows = [U.mixed_bytes(rng.randrange(0, 24), rng, weights=(1, 0, 0, 0, 0), words=[w for w in WORDS if w.isascii()]) for _ in range(2000)]
    one = list(ascii_rows)
    one[1234] = "a😀c привет 7".encode()
    return {"mixed": U.Expected(mixed), "ascii": U.Expected(ascii_rows), "one non-ASCII row": U.Expected(one)}  # (decoded once, shared)


def oracle_spans(o, want):
    """Per row of an Expected: the oracle's matches on the row's decoded units, mapped to byte offsets; and its containedIn()."""
    spans, inside, uoff = [], [], want.unit_offsets()
    for r, bm in enumerate(want.byte_maps):
        units = np.ascontiguousarray(want.units[uoff[r]:uoff[r + 1]])
        spans.append([(bm[s], bm[e]) for s, e in o.find_all(units, limit=1 << 30)])
        inside.append(bool(o.contained_in(units)))
    return spans, np.array(inside)


def flat(spans):
    off = np.zeros(len(spans) + 1, np.int64)
    off[1:] = np.cumsum([len(x) for x in spans])
    return off, np.array([s for x in spans for s, _ in x], np.int32), np.array([e for x in spans for _, e in x], np.int32)


def same_list(got, want, what):
    for g, w, name in zip(got, want, ("offsets", "byte_start", "byte_end")):
        g = g.cpu().numpy() if not isinstance(g, np.ndarray) else g
        assert g.shape == w.shape and (g == w).all(), (name, what)


@pytest.mark.parametrize("regex,flags", PATTERNS, ids=[p for p, _ in PATTERNS])
def test_end_to_end(e2e_rows, regex, flags):
    import torch
    from needle_amd.pattern import pack_bytes, unpack_bitmap
    p, o = compiled(regex, flags)
    for name, decoded in e2e_rows.items():
        rows = decoded.rows
        spans, inside = oracle_spans(o, decoded)
        want = flat(spans)
        assert name != "mixed" or want[1].size > 0, "the batch has matches"
        data, offsets, host = U.device_utf8(rows)
        same_list(p.find_all_utf8_packed(data, offsets), want, ("device chain", name))
        assert (unpack_bitmap(p.contained_in_utf8_packed(data, offsets), len(rows)) == inside).all(), ("containedIn, device chain", name)
        torch.cuda.synchronize()
        hd, ho = pack_bytes(rows)
        same_list(p.find_all_utf8_packed(hd, ho), want, ("host entry", name))  # (the all-ASCII batch takes the host entry's 8-bit shortcut)
        words, mal = p.contained_in_utf8_packed(hd, ho, malformed=True)
        assert (unpack_bitmap(words, len(rows)) == inside).all(), ("containedIn, host entry", name)
        assert (mal == U.bitmap(decoded.malformed)).all(), ("malformed", name)
        if name == "ascii":
            # the same ASCII rows with the shortcut NOT taken: one non-ASCII row behind them in the same chunk
            tail = rows + ["é".encode()]
            td, to = pack_bytes(tail)
            off, st, en = p.find_all_utf8_packed(td, to)
            k = int(off[len(rows)])
            same_list((off[:len(rows) + 1], st[:k], en[:k]), want, "host entry, shortcut not taken")
            assert (unpack_bitmap(p.contained_in_utf8_packed(td, to), len(tail))[:len(rows)] == inside).all()
        if name != "mixed":
            sub, repl = rows[:600] + rows[1200:1300], "<é😀>".encode()
            got = p.replace_all_bytes(sub, repl)
            lists = spans[:600] + spans[1200:1300]
            for r, row in enumerate(sub):
                assert got[r] == splice(row, lists[r], repl), ("replace_all_bytes", name, r)
    mixed = e2e_rows["mixed"].rows[:1500]
    got = p.replace_all_bytes(mixed, b"")
    spans, _ = oracle_spans(o, U.Expected(mixed))
    assert all(got[r] == splice(row, spans[r], b"") for r, row in enumerate(mixed)), "replace_all_bytes deleting, ill-formed bytes untouched"


def test_the_eight_bit_entry_reads_another_text():
    """The motivating bug: on "café 123" the 8-bit entry sees Latin-1 chars, the UTF-8 entry the text.  (It cannot pass without the feature.)"""
    from needle_amd.pattern import pack_bytes
    p, o = compiled("é.")
    row = "café 123".encode("utf-8")
    found, s, e = o.find(np.array(U.utf8_units(row)[0], np.uint16))
    assert found and (s, e) == (3, 5)
    assert p.find_all_bytes([row]) == [[(U.byte_of_unit(row, s), U.byte_of_unit(row, e))]] == [[(3, 6)]]
    data, off = pack_bytes([row])
    _, st, en = p.find_packed(data, off)  # the bytes as Latin-1: "cafÃ© 123"
    assert (int(st[0]), int(en[0])) != (3, 6)


# ---- 6. the host find-all entry in several chunks, and its capacity protocol
HOST_CHILD = r'''
import ctypes, random
import numpy as np
from oracle import walker; walker.build()
import utf8_cases as U
from needle_amd import _lib
from needle_amd.pattern import pack_bytes
from test_gpu_configs import compiled
from test_gpu_utf8 import WORDS, flat, oracle_spans
from test_host_plan import packed_chunks
L = _lib.lib()
rng = random.Random(23)
rows = [U.mixed_bytes(rng.randrange(0, 40), rng, words=WORDS) for _ in range(400)] + [b"plain ascii 7 rows 2024"] * 130
p, o = compiled("[0-9]+|[а-я]+|a.c")
spans, _ = oracle_spans(o, U.Expected(rows))
want = flat(spans)
data, off = pack_bytes(rows)
chunks = packed_chunks([int(x) for x in off], 1, 8 + 8 + 8 + 4 + 8 + 1, 64, 4096)
assert len(chunks) >= 4
v = _lib.PackedView()
v.data, v.char_width, v.n_rows, v.offsets = data.ctypes.data, 1, len(rows), off.ctypes.data
def call(capacity, arrays=True):
    out, total = np.full(len(rows) + 1, 99, np.uint64), ctypes.c_uint64(99)
    st, en = np.full(max(capacity, 1), -7, np.int32), np.full(max(capacity, 1), -7, np.int32)
    mal = np.full((len(rows) + 63) // 64, 99, np.uint64)
    rc = L.needle_find_all_csr_utf8_packed_host(p._h, ctypes.byref(v), out.ctypes.data, st.ctypes.data if arrays else None, en.ctypes.data if arrays else None,
                                                capacity, ctypes.byref(total), mal.ctypes.data)
    assert rc == 0, L.needle_last_error()
    return out.astype(np.int64), st, en, total.value, mal
m = want[1].size
out, st, en, total, mal = call(0, arrays=False)                      # the sizing call
assert total == m and (out == want[0]).all()
assert (mal == U.bitmap(U.Expected(rows).malformed)).all()
out, st, en, total, mal = call(m)                                    # the exact second call
assert total == m and (out == want[0]).all() and (st == want[1]).all() and (en == want[2]).all()
r_fit = chunks[1][1]                                                 # two chunks fit, the third does not
cap = int(want[0][r_fit]) + 1
assert cap < int(want[0][chunks[2][1]])
out, st, en, total, mal = call(cap)
k = int(want[0][r_fit])
assert total == m and (out == want[0]).all() and (st[:k] == want[1][:k]).all() and (en[:k] == want[2][:k]).all() and (st[k:] == -7).all() and (en[k:] == -7).all()
print("UTF8-HOST-OK")
'''


def test_host_entry_in_chunks_and_its_capacity_protocol():
    """6. NEEDLE_HOST_CHUNK_BYTES is read once per process, so a child process: 530 rows in chunks of 4 KiB (some all ASCII: the 8-bit
    shortcut beside the transcoding chunks), the sizing call, the exact call, and a capacity that ends between two chunks."""
    env = dict(os.environ, NEEDLE_HOST_CHUNK_BYTES="4096", NEEDLE_HOST_RESULT_BYTES="4096",
               PYTHONPATH=os.pathsep.join([ROOT, os.path.join(ROOT, "tests")] + os.environ.get("PYTHONPATH", "").split(os.pathsep)))
    r = subprocess.run([sys.executable, "-c", HOST_CHILD], env=env, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert "UTF8-HOST-OK" in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]
