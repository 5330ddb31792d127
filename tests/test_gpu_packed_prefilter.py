"""containedIn() / find() of PACKED device batches behind the n-gram candidate filter (needle_amd/csrc/needle_ngram_packed.h; routing:
choose_route / run_packed_dev in needle_api.cpp).  Every case is checked against the CPU oracle on every row (DFAClassBuilder.java:335-471, 625-659,
1004-1022 restated by oracle/) and, bit for bit, against the same call with the filter pinned OFF (the plain packed kernel of
needle_packed.h).  `filter_launches` of needle_pattern_prefilter_state says which kernel ran: it rises by one per packed call behind the
filter and does not move under OFF or with NEEDLE_PREFILTER_PACKED=0.

Layouts: every start offset mod 16, runs and whole groups of empty rows, keyword junk before offsets[0] and behind offsets[n] in the same
tensor (an over-read changes answers), offsets[0] = 0 and > 0, the last row at the tensor's end, partial and whole groups, only empty rows,
a batch of fewer than 16 bytes; keywords as whole rows, at a row's first and last chars, split over two rows (no match), two adjacent
one-keyword rows; rows of 70 000 and 1 MiB chars among 10 000 short ones; the 2- and 4-byte result forms with their escapes and overflow
flag; the flood watch; a non-default stream and out= buffers; 10^7 ragged rows; seeded random dictionaries, 8- and 16-bit."""
import os
import subprocess
import sys

import numpy as np
import pytest

from test_gpu_configs import compiled
from test_gpu_packed_dev import device_packed, layout_rows, oracle_packed

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LETTERS = [ord(ch) for ch in "abcdefghijklmnopqrstuvwxyz "]


def launches(p):
    return p.prefilter_state("forwards")["filter_launches"] + p.prefilter_state("contained_in")["filter_launches"]


def run_calls(p, data, offsets, stream=None):
    """The four packed calls the filter serves -> numpy (containedIn words, find words, start, end, dwords, dword overflow, uint16s,
    uint16 overflow)."""
    import torch
    c = p.contained_in_packed(data, offsets, stream=stream)
    fw, fs, fe = p.find_packed(data, offsets, stream=stream)
    w16, r16, o16 = p.find_packed16_packed(data, offsets, stream=stream)
    w8, r8, o8 = p.find_packed8_packed(data, offsets, stream=stream)
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in (c, fw, fs, fe, w16, r16, o16, w8, r8, o8)]


def check(p, o, rows, dtype, lead=5, trail=7, junk=None, mode=None, expect_filter=True, what=""):
    """The packed calls under `mode` (default: pinned ON -- AUTO has its own tests) against the oracle on every row and against the
    OFF route word for word; the launch counter moves by one per call, or not at all."""
    from needle_amd.pattern import Pattern, unpack_bitmap
    n = len(rows)
    data, offsets = device_packed(rows, dtype, lead, trail, junk)
    p.set_prefilter(p.PREFILTER_ON if mode is None else mode)
    before = launches(p)
    got = run_calls(p, data, offsets)
    moved = launches(p) - before
    assert (moved >= 4) if expect_filter else (moved == 0), (what, "filter launches", moved)
    p.set_prefilter(p.PREFILTER_OFF)
    before = launches(p)
    off = run_calls(p, data, offsets)
    assert launches(p) == before, (what, "OFF launched the filter kernel")
    p.set_prefilter(p.PREFILTER_AUTO)
    nw = (n + 63) // 64
    names = ("containedIn words", "find words", "start", "end", "words16", "dwords", "overflow16", "words8", "uint16s", "overflow8")
    for name, a, b in zip(names, got, off):
        k = nw if "words" in name else (n if name in ("start", "end", "dwords", "uint16s") else 1)
        bad = np.nonzero(a[:k] != b[:k])[0]
        assert bad.size == 0, (what, name, "differs from the OFF route", bad[:10], a[bad[:5]], b[bad[:5]])
    _, wc, wf, ws, we = oracle_packed(o, rows, dtype)
    c, fw, fs, fe, w16, r16, o16, w8, r8, o8 = got
    for name, g, w in (("containedIn", unpack_bitmap(c, n), wc), ("find", unpack_bitmap(fw, n), wf), ("start", fs[:n], ws), ("end", fe[:n], we),
                       ("find16", unpack_bitmap(w16, n), wf), ("find8", unpack_bitmap(w8, n), wf)):
        bad = np.nonzero(g != w)[0]
        assert bad.size == 0, (what, name, bad[:10], [len(rows[i]) for i in bad[:10]], g[bad[:5]], w[bad[:5]])
    # the one-word forms decode to the oracle's pairs; rows that do not fit carry the escape and raise the flag
    s16, e16, over16 = Pattern.unpack16_packed(r16[:n])
    fits16 = we <= 65534
    assert (over16 == (wf & ~fits16)).all() and (s16[fits16] == ws[fits16]).all() and (e16[fits16] == we[fits16]).all(), (what, "dword form")
    assert int(o16[0]) == int(over16.any()), (what, "dword overflow flag")
    s8, e8, over8 = Pattern.unpack8_packed(r8[:n])
    fits8 = we <= 256
    assert (over8 == (wf & ~fits8)).all() and (s8[fits8] == ws[fits8]).all() and (e8[fits8] == we[fits8]).all(), (what, "uint16 form")
    assert int(o8[0]) == int(over8.any()), (what, "uint16 overflow flag")
    return int(wf.sum())


def boundary_rows(rng, words, alphabet, dtype, n=400):
    """Keywords as whole rows, at a row's first / last chars, split over rows r / r + 1, two adjacent one-keyword rows, rows of 0 .. 3
    chars -- among ordinary rows."""
    al = np.asarray(alphabet)
    rows = []
    enc = lambda w: np.array([ord(ch) for ch in w], dtype=dtype)
    for i in range(n):
        w = enc(words[int(rng.integers(0, len(words)))])
        fill = lambda k: rng.choice(al, int(k)).astype(dtype)
        kind = i % 8
        if kind == 0:
            rows += [w, enc(words[int(rng.integers(0, len(words)))])]            # two adjacent one-keyword rows
        elif kind == 1:
            cut = int(rng.integers(1, w.size))
            rows += [np.concatenate([fill(rng.integers(0, 40)), w[:cut]]), np.concatenate([w[cut:], fill(rng.integers(0, 40))])]  # split: no match
        elif kind == 2:
            rows.append(np.concatenate([w, fill(rng.integers(0, 90))]))          # at the row's first chars
        elif kind == 3:
            rows.append(np.concatenate([fill(rng.integers(0, 90)), w]))          # at its last chars
        elif kind == 4:
            rows.append(fill(rng.integers(0, 4)))                                 # 0 .. 3 chars
        elif kind == 5:
            rows.append(np.concatenate([fill(rng.integers(0, 90)), w[:-1]]))     # cut by the row's end
        else:
            rows.append(fill(rng.integers(0, 200)))
    return rows


def layouts(p, o, words, alphabet, dtype, seed, n=1000, max_len=120):
    """Every layout of the list above for one pattern."""
    rng = np.random.default_rng(seed)
    junk = [ord(ch) for ch in words[0] + words[1]]
    rows = layout_rows(rng, alphabet, words, n=n, max_len=max_len, dtype=dtype)
    hits = check(p, o, rows, dtype, lead=5, trail=7, junk=junk, what="lead 5 trail 7")
    assert hits > 20
    check(p, o, rows, dtype, lead=0, trail=0, junk=junk, what="offsets[0] = 0, last row at the tensor's end")
    check(p, o, rows, dtype, lead=133, trail=0, junk=junk, what="offsets[0] > 0, last row at the tensor's end")
    for k in (1, 63, 64, 65, 130, 200):
        check(p, o, rows[48:48 + k], dtype, lead=3, trail=5, junk=junk, what="n_rows %d" % k)
    check(p, o, [np.zeros(0, dtype)] * 70, dtype, lead=9, trail=9, junk=junk, what="only empty rows")
    w = np.array([ord(ch) for ch in words[2]], dtype=dtype)
    tiny_n = 15 // np.dtype(dtype).itemsize
    for tiny in ([w[:tiny_n]], [np.zeros(0, dtype), w[:6], np.zeros(0, dtype), w[:1]], [w[:3], w[3:6]]):   # under 16 bytes in all
        assert sum(r.size for r in tiny) * np.dtype(dtype).itemsize < 16
        check(p, o, tiny, dtype, lead=0, trail=0, junk=junk, what="tiny batch, nothing around it")
        check(p, o, tiny, dtype, lead=21, trail=30, junk=junk, what="tiny batch inside keyword junk")
    # a keyword as the batch's LAST row (it starts inside the batch's last 16 chars: the verify walk's piece starts ahead of the row),
    # and batches just above the tiny limit
    wl = np.array([ord(ch) for ch in words[4]], dtype=dtype)
    for k in (70, 3):
        assert check(p, o, rows[48:48 + k] + [wl], dtype, lead=0, trail=0, junk=junk, what="keyword is the last row, tensor's end") >= 1
        check(p, o, rows[48:48 + k] + [wl, w[:2]], dtype, lead=2, trail=9, junk=junk, what="keyword in the batch's last 16 chars")
    fill = np.array(alphabet[:10], dtype=dtype)
    assert check(p, o, [np.concatenate([fill, wl])], dtype, lead=0, trail=0, junk=junk, what="one row of 16 .. 18 chars") == 1
    assert check(p, o, [fill[:5], np.zeros(0, dtype), wl, fill[:3]], dtype, lead=1, trail=0, junk=junk, what="four rows, 14 .. 16 chars") == 1
    b = boundary_rows(rng, words, alphabet, dtype)
    assert check(p, o, b, dtype, lead=7, trail=2, junk=junk, what="boundaries") > 100
    check(p, o, b[::-1], dtype, lead=0, trail=0, junk=junk, what="boundaries, reversed")


def sprinkle(rows16, rng):
    """The sprinkles of tests/test_gpu_prefilter_utf16.py: CJK chars, 0x0100 | c (a keyword char's low byte under another high byte), 0x00FF."""
    out = []
    for r in rows16:
        r = r.copy()
        m = rng.random(r.size) < 0.02
        r[m] = rng.integers(0x4E00, 0x9FFF, size=int(m.sum()), dtype=np.uint16)
        m = rng.random(r.size) < 0.02
        r[m] |= 0x0100
        m = rng.random(r.size) < 0.005
        r[m] = 0x00FF
        out.append(r)
    return out


def cyr(w):
    return "".join(chr(0x0430 + ord(c) - 97) for c in w)


# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_which_kernel_ran_auto_on_off():
    """AUTO on quiet text and ON take the filter kernel (one launch per call); OFF does not.  Fails without the packed route."""
    import torch
    from needle_amd import workload as W
    words = W.keywords(1000, min_len=6, max_len=8)
    p, o = compiled("|".join(words))
    host = W.keyword_batch(np, words, 3, 3000, 256)
    lens = (np.arange(3000) * 2654435761 % 256 + 1)
    rows = [host[i, :lens[i]] for i in range(3000)]
    data, offsets = device_packed(rows, np.uint8, 5, 7, None)
    _, wc, wf, ws, we = oracle_packed(o, rows, np.uint8)
    from needle_amd.pattern import unpack_bitmap
    for mode, per_call in ((p.PREFILTER_AUTO, 1), (p.PREFILTER_ON, 1), (p.PREFILTER_OFF, 0)):
        p.set_prefilter(mode)
        for _ in range(2):
            b = launches(p)
            fw, fs, fe = p.find_packed(data, offsets)
            torch.cuda.synchronize()
            assert launches(p) - b == per_call, (mode, "find_packed", launches(p) - b)
            b = launches(p)
            c = p.contained_in_packed(data, offsets)
            torch.cuda.synchronize()
            assert launches(p) - b == per_call, (mode, "contained_in_packed", launches(p) - b)
            assert (unpack_bitmap(fw, 3000) == wf).all() and (fs.cpu().numpy() == ws).all() and (fe.cpu().numpy() == we).all()
            assert (unpack_bitmap(c, 3000) == wc).all()
        # matches() and per-row cursors never take the filter
        b = launches(p)
        p.matches_packed(data, offsets)
        p.find_next_packed(data, offsets, torch.zeros(3000, dtype=torch.int32, device="cuda"))
        torch.cuda.synchronize()
        assert launches(p) == b
    p.set_prefilter(p.PREFILTER_AUTO)
    assert wf.sum() > 300


SWITCH_CHILD = r'''
import sys
sys.path.insert(0, "."); sys.path.insert(0, "tests")
import numpy as np, torch
from needle_amd import workload as W
import test_gpu_packed_prefilter as T
words = W.keywords(1000, min_len=6, max_len=8)
p, o = T.compiled("|".join(words))
rng = np.random.default_rng(2)
rows = T.layout_rows(rng, T.LETTERS, words, n=1500, max_len=200)
for mode in (p.PREFILTER_AUTO, p.PREFILTER_ON):
    T.check(p, o, rows, np.uint8, mode=mode, expect_filter=False, junk=[ord(c) for c in words[0]], what="NEEDLE_PREFILTER_PACKED=0")
assert T.launches(p) == 0
# the fixed-stride entries keep their filter
host = W.keyword_batch(np, words, 3, 20000, 256)
p.find_batch(torch.from_numpy(host).cuda())
torch.cuda.synchronize()
assert T.launches(p) == 1
print("SWITCH-CHILD-OK")
'''


@pytest.mark.gpu
def test_switch_keeps_packed_rows_on_the_plain_kernel():
    r = subprocess.run([sys.executable, "-c", SWITCH_CHILD], env=dict(os.environ, NEEDLE_PREFILTER_PACKED="0"), capture_output=True, text=True, timeout=900, cwd=ROOT)
    assert "SWITCH-CHILD-OK" in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]


@pytest.mark.gpu
@pytest.mark.parametrize("n_words,mode", [(1000, 6), (3000, None)])
def test_dictionaries_8bit(n_words, mode):
    """1000 keywords of 6 .. 8 chars: the compressed automaton in LDS; 3000: walks out of HBM / L2."""
    from needle_amd import workload as W
    words = W.keywords(n_words, min_len=6, max_len=8)
    p, o = compiled("|".join(words))
    km = p.info()["kernel_mode"]["forwards"]
    assert (km == mode) if mode is not None else (km in (3, 5)), km
    layouts(p, o, words, LETTERS, np.uint8, seed=n_words)


@pytest.mark.gpu
@pytest.mark.parametrize("n_words", [1000, 3000])
def test_dictionaries_utf16_one_page(n_words):
    """The same dictionaries on the Cyrillic page over UTF-16 rows: the page's byte program, text narrowed on load."""
    from needle_amd import workload as W
    words = [cyr(w) for w in W.keywords(n_words, min_len=6, max_len=8)]
    p, o = compiled("|".join(words))
    assert p.utf16_route() is not None and p.utf16_route()[0] == 4
    rng = np.random.default_rng(n_words + 1)
    al = [0x0430 + k for k in range(26)] + [32]
    rows = sprinkle(layout_rows(rng, al, words, n=1500, max_len=150, dtype=np.uint16), rng)
    junk = [ord(ch) for ch in words[0]]
    assert check(p, o, rows, np.uint16, lead=5, trail=7, junk=junk, what="cyrillic") > 20
    check(p, o, rows, np.uint16, lead=0, trail=0, junk=junk, what="cyrillic, tensor's ends")
    for k in (1, 63, 65, 130):
        check(p, o, rows[48:48 + k], np.uint16, lead=3, trail=5, junk=junk, what="cyrillic n_rows %d" % k)
    b = sprinkle(boundary_rows(rng, words, al, np.uint16), rng)
    check(p, o, b, np.uint16, lead=1, trail=0, junk=junk, what="cyrillic boundaries")
    check(p, o, [np.array([ord(ch) for ch in words[3]][:7], dtype=np.uint16)], np.uint16, lead=0, trail=0, junk=junk, what="cyrillic tiny")
    # ... and the Latin dictionary itself over UTF-16 rows (page 0)
    if n_words == 1000:
        lw = W.keywords(n_words, min_len=6, max_len=8)
        p0, o0 = compiled("|".join(lw))
        rows0 = sprinkle(layout_rows(rng, LETTERS, lw, n=1500, max_len=150, dtype=np.uint16), rng)
        assert check(p0, o0, rows0, np.uint16, lead=2, trail=0, junk=[ord(ch) for ch in lw[0]], what="latin over UTF-16") > 20


@pytest.mark.gpu
def test_mixed_scripts_wide_filter():
    """W.keywords_mixed(300) over W.mixed_keyword_batch rows: no single page -- the WIDE filter."""
    from needle_amd import workload as W
    words = W.keywords_mixed(300)
    p, o = compiled("|".join(words))
    assert p.utf16_route() is None
    host = W.mixed_keyword_batch(np, words, 4000, 3000, 256)
    rng = np.random.default_rng(9)
    lens = rng.integers(0, 257, 3000)
    lens[:48] = np.arange(48)
    lens[200:264] = 0
    rows = [host[i, :lens[i]].astype(np.uint16) for i in range(3000)]
    for i in range(0, 3000, 9):      # keywords of every script at both ends of rows
        w = np.array([ord(c) for c in words[(i * 5) % len(words)]], dtype=np.uint16)
        rows[i] = np.concatenate([w, rows[i], np.array([ord(c) for c in words[(i * 7 + 1) % len(words)]], dtype=np.uint16)])
    junk = [ord(ch) for ch in words[0] + words[1]]
    assert check(p, o, rows, np.uint16, lead=5, trail=7, junk=junk, what="mixed scripts") > 100
    check(p, o, rows, np.uint16, lead=0, trail=0, junk=junk, what="mixed scripts, tensor's ends")
    for k in (1, 64, 130):
        check(p, o, rows[48:48 + k], np.uint16, lead=3, trail=5, junk=junk, what="mixed n_rows %d" % k)
    al = [ord(c) for w in words[:40] for c in w] + [32]
    check(p, o, boundary_rows(rng, words, al, np.uint16), np.uint16, lead=1, trail=0, junk=junk, what="mixed boundaries")


@pytest.mark.gpu
def test_pattern_with_char_ff_and_union_without_filter():
    """`abcdefÿgh|bcdefgh` takes whatever route choose_route gives it (a filter at NEEDLE_PREFILTER=2 only); the six-name union has no filter:
    the route declines and filter_launches stays put."""
    rng = np.random.default_rng(4)
    p, o = compiled("abcdefÿgh|bcdefgh")
    al = [ord(c) for c in "abcdefgh x"] + [0xFF]
    rows = layout_rows(rng, al, ["abcdefÿgh", "bcdefgh"], n=1000, max_len=120, dtype=np.uint16)
    on = bool(p.prefilter_info("forwards")["on"]) and p.utf16_route() is not None
    check(p, o, rows, np.uint16, junk=[ord(c) for c in "bcdefgh"], expect_filter=on, what="char 0xFF, UTF-16")
    rows8 = [r.astype(np.uint8) for r in rows]
    check(p, o, rows8, np.uint8, junk=[ord(c) for c in "bcdefgh"], expect_filter=bool(p.prefilter_info("forwards")["on"]), what="char 0xFF, 8-bit")
    names = ["Sherlock", "Holmes", "Watson", "Moriarty", "Mycroft", "Baskerville"]
    p, o = compiled("|".join(names))
    assert p.prefilter_info("forwards")["on"] == 0
    rows = layout_rows(rng, [ord(c) for c in "SherlockHmsWatnMiyfBv "], names, n=1000, max_len=120)
    for mode in (p.PREFILTER_AUTO, p.PREFILTER_ON):
        assert check(p, o, rows, np.uint8, junk=[ord(c) for c in "Holmes"], mode=mode, expect_filter=False, what="six names") > 20
    assert launches(p) == 0


FF_CHILD = r'''
import sys
sys.path.insert(0, "."); sys.path.insert(0, "tests")
import numpy as np
import test_gpu_packed_prefilter as T
rng = np.random.default_rng(4)
p, o = T.compiled("abcdefÿgh|bcdefgh")
assert p.prefilter_info("forwards")["on"] and p.utf16_route() is not None
al = [ord(c) for c in "abcdefgh x"] + [0xFF]
rows = T.layout_rows(rng, al, ["abcdefÿgh", "bcdefgh"], n=1500, max_len=120, dtype=np.uint16)
assert T.check(p, o, rows, np.uint16, junk=[ord(c) for c in "bcdefgh"], what="char 0xFF, UTF-16") > 20
assert T.check(p, o, [r.astype(np.uint8) for r in rows], np.uint8, junk=[ord(c) for c in "bcdefgh"], what="char 0xFF, 8-bit") > 20
T.check(p, o, T.boundary_rows(rng, ["abcdefÿgh", "bcdefgh"], al, np.uint16), np.uint16, lead=0, trail=0, what="char 0xFF boundaries")
print("FF-CHILD-OK")
'''


@pytest.mark.gpu
def test_pattern_with_char_ff_behind_the_filter():
    """NEEDLE_PREFILTER=2 (filters for plain LDS tables too): the pattern with a char at 0xFF behind the packed filter, 8- and 16-bit."""
    r = subprocess.run([sys.executable, "-c", FF_CHILD], env=dict(os.environ, NEEDLE_PREFILTER="2", NEEDLE_PAIR_MAX_BYTES="0"), capture_output=True, text=True,
                       timeout=900, cwd=ROOT)
    assert "FF-CHILD-OK" in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]


@pytest.mark.gpu
def test_long_rows():
    """Rows of 70 000 and 1 MiB chars among 10 000 short ones: they are filtered like any other text (32-bit slot keys); int32 start /
    end exact before and beyond position 65 535 and at the row's last chars, and exact for the other 63 rows of such a group."""
    from needle_amd import workload as W
    words = W.keywords(1000, min_len=6, max_len=8)
    p, o = compiled("|".join(words))
    rng = np.random.default_rng(17)
    al = np.array(LETTERS, dtype=np.uint8)
    enc = lambda w: np.array([ord(ch) for ch in w], dtype=np.uint8)

    def long_row(n, where):
        r = rng.choice(al, n).astype(np.uint8)
        if where == "before":
            r[1000:1000 + len(words[5])] = enc(words[5])
        elif where == "beyond":
            r[65536 + 77:65536 + 77 + len(words[6])] = enc(words[6])
        elif where == "straddle":
            r[65535 - 3:65535 - 3 + len(words[7])] = enc(words[7])
        elif where == "end":
            r[n - len(words[8]):] = enc(words[8])
        return r
    longs = [long_row(n, w) for n in (70000, 1 << 20) for w in ("before", "beyond", "straddle", "end", "none")]
    short = layout_rows(rng, LETTERS, words, n=10000, max_len=60)
    rows = list(short)
    for k, r in enumerate(longs):
        rows.insert(37 + k * 811, r)
    junk = [ord(ch) for ch in words[0]]
    assert check(p, o, rows, np.uint8, lead=13, trail=9, junk=junk, what="long among short") > 1000
    check(p, o, longs, np.uint8, lead=1, trail=0, junk=junk, what="long rows only")
    cw = [cyr(w) for w in words]
    pc, oc = compiled("|".join(cw))
    rows16 = [np.where(r >= 97, r.astype(np.uint16) + (0x0430 - 97), r.astype(np.uint16)).astype(np.uint16) for r in rows[:3000]]
    assert check(pc, oc, rows16, np.uint16, lead=1, trail=3, junk=[ord(ch) for ch in cw[0]], what="long among short, 16-bit") > 300


@pytest.mark.gpu
def test_flood_watch_on_packed_text():
    """The flood text of tests/test_gpu_prefilter_watch.py, packed with ragged lengths: the state flips to suspended after the first
    evaluated launch; ON never suspends; the answers are the oracle's in every state."""
    import torch
    from needle_amd import workload as W
    from needle_amd.pattern import unpack_bitmap
    words = W.keywords(1000, min_len=6, max_len=8)
    p, o = compiled("|".join(words))
    n, stride = 64 * 200 + 9, 256
    rng = np.random.default_rng(5)
    long_words = [w for w in words if len(w) >= 6][:512]
    wt8 = np.full((len(long_words), 8), 32, dtype=np.uint8)
    for i, w in enumerate(long_words):
        t = np.array([ord(c) for c in w[-8:]], dtype=np.uint8)
        t[0] = ord("q") if t[0] != ord("q") else ord("z")
        wt8[i, 8 - t.size:] = t
    flood = wt8[rng.integers(0, len(long_words), (n, stride // 8))].reshape(n, stride).copy()
    flood[::5, 8:8 + len(words[0])] = [ord(c) for c in words[0]]
    lens = rng.integers(100, stride + 1, n)    # ragged; every call still gives the watch more than the 1024 KiB it evaluates on
    assert lens.sum() > (1100 << 10)
    frows = [flood[i, :lens[i]] for i in range(n)]
    quiet = W.keyword_batch(np, words, 9, n, stride)
    qrows = [quiet[i, :lens[i]] for i in range(n)]
    fd, fo = device_packed(frows, np.uint8, 3, 5, None)
    qd, qo = device_packed(qrows, np.uint8, 3, 5, None)
    want = {id(fd): oracle_packed(o, frows, np.uint8), id(qd): oracle_packed(o, qrows, np.uint8)}

    def call(d, offs):
        fw, fs, fe = p.find_packed(d, offs)
        torch.cuda.synchronize()
        _, _, wf, ws, we = want[id(d)]
        assert (unpack_bitmap(fw, n) == wf).all() and (fs.cpu().numpy() == ws).all() and (fe.cpu().numpy() == we).all()

    st = p.prefilter_state("forwards")
    assert st["mode"] == p.PREFILTER_AUTO and st["filter_launches"] == 0
    call(fd, fo)                                   # launch 1: the filter kernel; its counters arrive behind it
    st = p.prefilter_state("forwards")
    assert st["has_filter"] == 1 and st["filter_launches"] == 1 and st["suspended_calls_left"] == 0, st
    call(fd, fo)                                   # call 2 evaluates launch 1: flooded -> this call and the next 31 take the plain packed kernel
    st = p.prefilter_state("forwards")
    assert st["last_candidates_per_kib"] > 16 and st["suspended_calls_left"] == 31 and st["backoff"] == 64 and st["filter_launches"] == 1, st
    for _ in range(31):
        p.find_packed(qd, qo)
    torch.cuda.synchronize()
    st = p.prefilter_state("forwards")
    assert st["suspended_calls_left"] == 0 and st["suspended_calls"] == 32 and st["filter_launches"] == 1, st
    call(qd, qo)                                   # the filter is tried again ...
    call(qd, qo)                                   # ... and found quiet
    st = p.prefilter_state("forwards")
    assert st["filter_launches"] == 3 and st["last_candidates_per_kib"] < 16 and st["backoff"] == 32 and st["suspended_calls_left"] == 0, st
    p.set_prefilter(p.PREFILTER_ON)                # pinned ON: flood text through the filter kernel every time, never suspended
    for _ in range(3):
        call(fd, fo)
    st = p.prefilter_state("forwards")
    assert st["mode"] == p.PREFILTER_ON and st["filter_launches"] == 6 and st["suspended_calls_left"] == 0, st
    p.set_prefilter(p.PREFILTER_OFF)
    call(fd, fo)
    call(qd, qo)
    assert p.prefilter_state("forwards")["filter_launches"] == 6
    p.set_prefilter(p.PREFILTER_AUTO)


@pytest.mark.gpu
def test_non_default_stream_and_out_buffers():
    import torch
    from needle_amd import workload as W
    from needle_amd.pattern import unpack_bitmap
    words = W.keywords(1000, min_len=6, max_len=8)
    p, o = compiled("|".join(words))
    p.set_prefilter(p.PREFILTER_ON)
    rng = np.random.default_rng(31)
    rows = layout_rows(rng, LETTERS, words, n=5000, max_len=300)
    n = len(rows)
    s = torch.cuda.Stream()
    b = launches(p)
    with torch.cuda.stream(s):
        data, offsets = device_packed(rows, np.uint8, 3, 3, [ord(c) for c in words[0]])
        c = p.contained_in_packed(data, offsets, stream=s.cuda_stream)
        fw, fs, fe = p.find_packed(data, offsets, stream=s.cuda_stream)
    s.synchronize()
    assert launches(p) - b == 2
    _, wc, wf, ws, we = oracle_packed(o, rows, np.uint8)
    assert (unpack_bitmap(c, n) == wc).all() and (unpack_bitmap(fw, n) == wf).all()
    assert (fs.cpu().numpy() == ws).all() and (fe.cpu().numpy() == we).all()
    bm = torch.full(((n + 63) // 64,), -1, dtype=torch.int64, device="cuda")
    st = torch.empty(n, dtype=torch.int32, device="cuda")
    en = torch.empty(n, dtype=torch.int32, device="cuda")
    r = p.find_packed(data, offsets, out=(bm, st, en))
    torch.cuda.synchronize()
    assert launches(p) - b == 3
    assert r[0] is bm and (unpack_bitmap(bm, n) == wf).all() and (st.cpu().numpy() == ws).all() and (en.cpu().numpy() == we).all()
    p.set_prefilter(p.PREFILTER_AUTO)


@pytest.mark.gpu
def test_ten_million_ragged_rows():
    """10^7 ragged rows of the 1000-keyword dictionary (6 .. 8 chars), lengths (r * 2654435761) % 256 + 1, packed: the filter route equals
    the OFF route on every row and the oracle on 3000 sampled rows."""
    import torch
    from needle_amd import workload as W
    from needle_amd.pattern import unpack_bitmap
    n = 10_000_000
    dev = torch.device("cuda")
    lens = (torch.arange(n, device=dev, dtype=torch.int64) * 2654435761 % 256 + 1)
    offsets = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    offsets[1:] = torch.cumsum(lens, 0)
    col = torch.arange(256, device=dev)[None, :]
    sample = torch.from_numpy(np.random.default_rng(1).choice(n, 3000, replace=False)).to(dev)
    words = W.keywords(1000, min_len=6, max_len=8)
    p, o = compiled("|".join(words))
    rows = torch.empty((n, 256), dtype=torch.uint8, device=dev)
    for s in range(0, n, 1 << 19):
        k = min(1 << 19, n - s)
        rows[s:s + k] = W.keyword_batch(torch, words, s, k, 256, device=dev)
    data = torch.empty(int(offsets[-1].item()), dtype=torch.uint8, device=dev)
    for s in range(0, n, 1 << 20):
        k = min(1 << 20, n - s)
        data[int(offsets[s].item()):int(offsets[s + k].item())] = rows[s:s + k][col < lens[s:s + k, None]]
    srows = rows[sample].cpu().numpy()
    del rows
    b = launches(p)
    gw, gs, ge = p.find_packed(data, offsets)
    gc = p.contained_in_packed(data, offsets)
    torch.cuda.synchronize()
    assert launches(p) - b == 2
    p.set_prefilter(p.PREFILTER_OFF)
    ww, ws, we = p.find_packed(data, offsets)
    wc = p.contained_in_packed(data, offsets)
    torch.cuda.synchronize()
    p.set_prefilter(p.PREFILTER_AUTO)
    assert launches(p) - b == 2
    assert torch.equal(gw, ww) and torch.equal(gs, ws) and torch.equal(ge, we) and torch.equal(gc, wc)
    slens = lens[sample].cpu().numpy().astype(np.uint32)
    idx = sample.cpu().numpy()
    of, os_, oe = o.batch_find(srows, slens, threads=8)
    assert of.sum() > 300
    assert (unpack_bitmap(gw, n)[idx] == of).all() and (unpack_bitmap(gc, n)[idx] == of).all()
    assert (gs[sample].cpu().numpy() == os_).all() and (ge[sample].cpu().numpy() == oe).all()


FUZZ_CHILD = r'''
import sys, random
sys.path.insert(0, "."); sys.path.insert(0, "tests")
import numpy as np
import test_gpu_packed_prefilter as T
seed = int(sys.argv[1])
rng = random.Random(7000 + seed)
nrng = np.random.default_rng(seed)
letters = "abcdefgh"
redrawn = 0
while True:   # a dictionary without a filter is redrawn, not skipped
    words = sorted({"".join(rng.choice(letters) for _ in range(rng.randint(5, 9))) for _ in range(rng.randint(5, 60))})
    rng.shuffle(words)
    p, o = T.compiled("|".join(words))
    if p.prefilter_info("forwards")["on"] and p.prefilter_info("contained_in")["on"]:
        break
    redrawn += 1
    assert redrawn < 50
al = [ord(ch) for ch in letters + " "]
junk = [ord(ch) for ch in words[0]]
rows = T.layout_rows(nrng, al, words, n=1500, max_len=200)
hits = T.check(p, o, rows, np.uint8, lead=int(nrng.integers(0, 9)), trail=3, junk=junk, what=("dictionary", seed, words[:5]))
rows16 = T.sprinkle(T.layout_rows(nrng, al, words, n=1500, max_len=200, dtype=np.uint16), nrng)
hits += T.check(p, o, rows16, np.uint16, lead=int(nrng.integers(0, 9)), trail=int(nrng.integers(0, 2)) * 5, junk=junk, what=("dictionary 16-bit", seed, words[:5]))
T.check(p, o, T.boundary_rows(nrng, words, al, np.uint8), np.uint8, lead=int(nrng.integers(0, 17)), trail=0, junk=junk, what=("boundaries", seed))
assert hits > 50
print("FUZZ-CHILD-OK", redrawn)
'''


@pytest.mark.gpu
@pytest.mark.parametrize("seed", range(6))
def test_fuzz_random_dictionaries(seed):
    """Seeded random dictionaries (words of 5 .. 9 chars) over random packed batches, 8- and 16-bit, at NEEDLE_PREFILTER=2 so that small
    automata carry a filter too (read once per process: a child)."""
    r = subprocess.run([sys.executable, "-c", FUZZ_CHILD, str(seed)], env=dict(os.environ, NEEDLE_PREFILTER="2", NEEDLE_PAIR_MAX_BYTES="0"), capture_output=True,
                       text=True, timeout=900, cwd=ROOT)
    assert "FUZZ-CHILD-OK" in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]


def many_short_rows(words, dtype, n, seed):
    """(host text, offsets, lens) of n rows whose 64-row groups differ in size: most groups hold rows of 0 .. 40 chars (one 4 KiB batch of
    the filter's stream), every third group rows of 0 .. 300 chars (three batches), every seventh group only empty rows -- so a wave that
    owns several groups meets one-batch groups behind and in front of longer ones, and runs of them.  Keywords are planted in a fifth of the
    rows that can hold one."""
    rng = np.random.default_rng(seed)
    grp = np.arange(n) // 64
    hi = np.where(grp % 3 == 0, 301, 41)
    lens = (rng.random(n) * hi).astype(np.int64)
    lens[grp % 7 == 3] = 0
    lens[(grp % 11 == 5) & (np.arange(n) % 64 != 9)] = 0          # ... and groups with a single row
    offsets = np.zeros(n + 1, dtype=np.int64)
    offsets[1:] = np.cumsum(lens)
    text = rng.choice(np.array(LETTERS, dtype=dtype), int(offsets[-1]))
    enc = [np.array([ord(ch) for ch in w], dtype=dtype) for w in words]
    for r in np.nonzero((lens >= 8) & (rng.random(n) < 0.2))[0]:
        w = enc[int(rng.integers(0, len(enc)))]
        at = int(offsets[r]) + int(rng.integers(0, lens[r] - w.size + 1))
        text[at:at + w.size] = w
    return text, offsets, lens


@pytest.mark.gpu
@pytest.mark.parametrize("cw", [1, 2])
def test_many_groups_per_wave_with_one_batch_groups(cw):
    """10^6 rows = 15 625 groups: more than two groups for every wave the GPU holds (16 waves per CU), so the prefetch cursor -- up to two
    batches ahead of the batch being filtered -- crosses one-batch groups, empty groups and runs of them behind longer ones.  The filter
    route equals the OFF route on every row, and the oracle on 4000 sampled rows."""
    import torch
    from needle_amd import workload as W
    from needle_amd.pattern import unpack_bitmap
    n = 1_000_000
    assert (n + 63) // 64 > 3 * 16 * torch.cuda.get_device_properties(0).multi_processor_count
    latin = W.keywords(1000, min_len=6, max_len=8)
    dtype = np.uint8 if cw == 1 else np.uint16
    words = latin if cw == 1 else [cyr(w) for w in latin]
    p, o = compiled("|".join(words))
    text, offsets, lens = many_short_rows(latin, dtype, n, 40 + cw)
    if cw == 2:                              # the letters -- the planted keywords with them -- move to the Cyrillic page
        text = np.where(text >= 97, text + (0x0430 - 97), text).astype(np.uint16)
    pad = (-text.size * cw) % 4 // cw
    host = np.concatenate([text, np.zeros(pad, dtype)])
    data = torch.from_numpy(host.view(np.uint8) if cw == 1 else host.view(np.int16)).cuda()
    doff = torch.from_numpy(offsets).cuda()
    p.set_prefilter(p.PREFILTER_ON)
    b = launches(p)
    gw, gs, ge = p.find_packed(data, doff)
    gc = p.contained_in_packed(data, doff)
    torch.cuda.synchronize()
    assert launches(p) - b == 2
    p.set_prefilter(p.PREFILTER_OFF)
    ww, ws, we = p.find_packed(data, doff)
    wc = p.contained_in_packed(data, doff)
    torch.cuda.synchronize()
    p.set_prefilter(p.PREFILTER_AUTO)
    for name, a, w_ in (("find words", gw, ww), ("start", gs, ws), ("end", ge, we), ("containedIn words", gc, wc)):
        bad = torch.nonzero(a != w_).flatten()[:10].cpu().numpy()
        assert bad.size == 0, (name, "differs from the OFF route", bad, bad // 64 if "words" not in name else bad)
    idx = np.sort(np.random.default_rng(3).choice(n, 4000, replace=False))
    rows = [text[offsets[i]:offsets[i + 1]] for i in idx]
    _, oc, of, os_, oe = oracle_packed(o, rows, dtype)
    assert of.sum() > 100
    assert (unpack_bitmap(gw, n)[idx] == of).all() and (unpack_bitmap(gc, n)[idx] == oc).all()
    assert (gs.cpu().numpy()[idx] == os_).all() and (ge.cpu().numpy()[idx] == oe).all()


DIRECT_CHILD = r'''
import sys
sys.path.insert(0, "."); sys.path.insert(0, "tests")
import numpy as np
from needle_amd import workload as W
import test_gpu_packed_prefilter as T
words = W.keywords(1000, min_len=6, max_len=8)
p, o = T.compiled("|".join(words))
rng = np.random.default_rng(12)
junk = [ord(c) for c in words[0]]
# spans of 64 rows above 2000 chars are walked row by row (unaligned 16-char reads, positions far beyond one piece); the groups of
# empty and short rows between them are filtered: both kinds on one wave when the batch is long enough
rows = T.layout_rows(rng, T.LETTERS, words, n=3000, max_len=120)
rows[700] = np.concatenate([rng.choice(np.array(T.LETTERS, dtype=np.uint8), 70000), np.array([ord(c) for c in words[9]], dtype=np.uint8)])
assert T.check(p, o, rows, np.uint8, lead=5, trail=7, junk=junk, what="direct groups among filtered ones") > 100
T.check(p, o, rows, np.uint8, lead=0, trail=0, junk=junk, what="direct groups, tensor's ends")
T.check(p, o, T.boundary_rows(rng, words, T.LETTERS, np.uint8), np.uint8, lead=3, trail=0, junk=junk, what="direct groups, boundaries")
cw = [T.cyr(w) for w in words]
pc, oc = T.compiled("|".join(cw))
rows16 = T.sprinkle([np.where(r >= 97, r.astype(np.uint16) + (0x0430 - 97), r.astype(np.uint16)).astype(np.uint16) for r in rows[:1500]], rng)
assert T.check(pc, oc, rows16, np.uint16, lead=1, trail=0, junk=[ord(c) for c in cw[0]], what="direct groups, 16-bit") > 50
wm = W.keywords_mixed(300)
pm, om = T.compiled("|".join(wm))
host = W.mixed_keyword_batch(np, wm, 4000, 1500, 256)
lens = rng.integers(0, 257, 1500)
assert T.check(pm, om, [host[i, :lens[i]].astype(np.uint16) for i in range(1500)], np.uint16, lead=2, trail=3, what="direct groups, wide") > 50
print("DIRECT-CHILD-OK")
'''


@pytest.mark.gpu
def test_row_by_row_walk_of_groups_beyond_the_stream_positions():
    """The walk that serves groups whose span exceeds the kernel's 32-bit stream positions (more than 2 GiB of text in 64 rows: nothing a
    test can hold), reached by lowering its threshold: NEEDLE_PACKED_DIRECT_ABOVE=2000 (read once per process: a child)."""
    r = subprocess.run([sys.executable, "-c", DIRECT_CHILD], env=dict(os.environ, NEEDLE_PACKED_DIRECT_ABOVE="2000"), capture_output=True, text=True,
                       timeout=900, cwd=ROOT)
    assert "DIRECT-CHILD-OK" in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]
