"""The per-lane packed find-all kernel (needle_packed_find_all_lane.h): every match of every packed row for patterns WITHOUT a find-all
transducer -- nullable patterns, unbounded ones with backward walks, nested dictionaries -- through needle_count_matches_packed_dev /
needle_find_all_csr_packed_dev, bit-exact against the oracle's repeated find(), the fixed-stride entries and the host entry
(check_all of tests/test_gpu_find_all_packed.py).  Every test first asserts that the route is "lane"."""
import ctypes
import random

import numpy as np
import pytest

from test_gpu_configs import compiled
from test_gpu_find_all_packed import check_all, flatten, oracle_all
from test_gpu_packed_dev import device_packed, layout_rows

LONG = "ab" + "c" * 300 + "d|ab"
PATTERNS = [
    # (regex, char width, alphabet, planted words, junk that matches)
    ("international|inter|nation", 1, "interntiol ", ["international", "inter", "nation"], "inter"),
    ("[a-c]*", 1, "abcd", [], "abc"),
    ("http://.+", 1, "htp:/abc.x\n", ["http://", "http://a.b"], "http://x"),
    ("abc+d|ab", 1, "abcd x", ["abccd", "ab", "abcccc"], "abcd"),
    (LONG, 1, "abcd", ["ab", "ab" + "c" * 300 + "d", "ab" + "c" * 50], "ab"),
    ("[a-z一-丠]+[0-9]|ЖЗ+", 2, "az9一丐丰ЖЗ ", ["一丁x7", "ЖЗЗ"], "一a1"),
]


def assert_lane(p, cw):
    assert p.find_all_packed_route(cw, False) == "lane" and p.find_all_packed_route(cw, True) == "lane"


def codes(s, dtype):
    return np.array([ord(c) for c in s], dtype)


@pytest.mark.gpu
@pytest.mark.parametrize("regex,cw,alphabet,plants,junk", PATTERNS)
def test_layouts(regex, cw, alphabet, plants, junk):
    p, o = compiled(regex)
    assert_lane(p, cw)
    dtype = np.uint8 if cw == 1 else np.uint16
    rng = np.random.default_rng(23 + len(regex))
    al = [ord(ch) for ch in alphabet]
    jk = [ord(ch) for ch in junk]
    rows = layout_rows(rng, al, plants, n=700, max_len=120, dtype=dtype)
    for lead, trail in ((5, 7), (0, 0), (133, 0)):
        check_all(p, o, rows, dtype, lead=lead, trail=trail, junk=jk, kernel=False, what="lead %d trail %d" % (lead, trail))
    for n in (1, 63, 65, 130):                      # batches ending inside a 64-row group
        check_all(p, o, rows[48:48 + n], dtype, lead=3, trail=5, junk=jk, what="n_rows %d" % n)
    check_all(p, o, [np.zeros(0, dtype)] * 70, dtype, lead=9, trail=9, junk=jk, what="only empty rows")


@pytest.mark.gpu
@pytest.mark.parametrize("cw", [1, 2])
def test_restarts_across_windows_bounded_lengths(cw):
    """A search dies 301 chars behind its restart point: nearly every 4 / 8 KiB window edge falls inside a restart gap."""
    p, o = compiled(LONG)
    assert_lane(p, cw)
    dtype = np.uint8 if cw == 1 else np.uint16
    period = codes("ab" + "c" * 300 + "x", dtype)
    one = np.resize(period, 20000)
    assert o.find_all(one, limit=1 << 30) == [(303 * k, 303 * k + 2) for k in range(67)]
    rng = np.random.default_rng(4)
    short = layout_rows(rng, [ord(c) for c in "abcd"], ["ab", "ab" + "c" * 40], n=100, max_len=90, dtype=dtype)
    long_rows = [np.resize(np.roll(period, -i), 20000).astype(dtype) for i in range(64)]  # row i starts at char i of the period
    three = codes(("ab" + "c" * 300 + "d") * 3 + "ab", dtype)
    assert o.find_all(three, limit=1 << 30) == [(0, 303), (303, 606), (606, 909), (909, 911)]
    pending = np.concatenate([codes("xx", dtype), np.resize(period, 3 * 303), codes("ab" + "c" * 100, dtype)])
    assert o.find_all(pending, limit=1 << 30)[-1] == (911, 913)
    rows = []
    for i in range(64):
        rows.append(short[i])
        rows.append(long_rows[i])
    rows += short[64:] + [three, pending]
    check_all(p, o, rows, dtype, lead=7, trail=3, junk=[ord("a"), ord("b")], kernel=False)


DEFER_ROW = ("ab" + "c" * 5000 + "x") * 3 + "abccd" + "ab"
DEFER_WANT = [(0, 2), (5003, 5005), (10006, 10008), (15009, 15014), (15014, 15016)]


@pytest.mark.gpu
@pytest.mark.parametrize("cw", [1, 2])
def test_restart_further_back_than_a_window_deferred_starts(cw):
    p, o = compiled("abc+d|ab")
    assert_lane(p, cw)
    dtype = np.uint8 if cw == 1 else np.uint16
    row = codes(DEFER_ROW, dtype)
    assert o.find_all(row, limit=1 << 30) == DEFER_WANT
    rng = np.random.default_rng(9)
    short = layout_rows(rng, [ord(c) for c in "abcd x"], ["abccd", "ab"], n=150, max_len=100, dtype=dtype)
    jk = [ord(c) for c in "abcd"]
    check_all(p, o, [row], dtype, lead=5, trail=7, junk=jk, kernel=False, what="the only row")
    check_all(p, o, [row] + short[:80], dtype, lead=0, trail=0, junk=jk, what="row 0")
    check_all(p, o, short[:63] + [row] + short[63:90], dtype, lead=3, trail=1, junk=jk, what="row 63")
    check_all(p, o, short[:70] + [row] + short[70:], dtype, lead=11, trail=2, junk=jk, what="among short rows")


@pytest.mark.gpu
def test_nested_text_every_lead():
    p, o = compiled("international|inter|nation")
    assert_lane(p, 1)
    row = np.resize(codes("internationa ", np.uint8), 6000)
    for lead in range(16):
        check_all(p, o, [row, row[:77], row], np.uint8, lead=lead, trail=4, junk=[ord(c) for c in "inter"], what="lead %d" % lead)


@pytest.mark.gpu
def test_capacity_more_and_canary():
    """Offsets with room for at most one match per row: more = 1, every row's first match filed, nothing written past the offsets."""
    import torch
    from needle_amd import _lib
    p, o = compiled("abc+d|ab")
    assert_lane(p, 1)
    rng = np.random.default_rng(12)
    rows = layout_rows(rng, [ord(c) for c in "abcd "], ["abccd", "ab"], n=300, max_len=120)
    rows[7] = codes("ab abcd ab ab abccccd", np.uint8)
    want = oracle_all(o, rows)
    counts = np.array([len(x) for x in want])
    assert (counts > 1).sum() > 50
    data, offsets = device_packed(rows, np.uint8, lead=5, trail=7, junk=[ord("a"), ord("b")])
    room = np.minimum(counts, 1)
    off = np.zeros(len(rows) + 1, np.int64)
    off[1:] = np.cumsum(room)
    total = int(off[-1])
    CANARY = -1234567
    st = torch.full((total + 64,), CANARY, dtype=torch.int32, device="cuda")
    en = torch.full((total + 64,), CANARY, dtype=torch.int32, device="cuda")
    d_off = torch.from_numpy(off).to("cuda")
    v = p._packed_dev_view(data, offsets)
    more = ctypes.c_int(0)
    s = torch.cuda.current_stream().cuda_stream
    rc = _lib.lib().needle_find_all_csr_packed_dev(p._h, ctypes.byref(v), d_off.data_ptr(), st.data_ptr(), en.data_ptr(), ctypes.byref(more), s)
    assert rc == 0 and more.value == 1
    torch.cuda.synchronize()
    st, en = st.cpu().numpy(), en.cpu().numpy()
    first = [x[0] for x in want if x]
    assert st[:total].tolist() == [a for a, _ in first] and en[:total].tolist() == [b for _, b in first]
    assert (st[total:] == CANARY).all() and (en[total:] == CANARY).all()
    # exact room: more stays 0
    full = flatten(want)
    st2 = torch.full((int(full[0][-1]) + 64,), CANARY, dtype=torch.int32, device="cuda")
    en2 = torch.full((int(full[0][-1]) + 64,), CANARY, dtype=torch.int32, device="cuda")
    d_off2 = torch.from_numpy(full[0]).to("cuda")
    more = ctypes.c_int(1)
    rc = _lib.lib().needle_find_all_csr_packed_dev(p._h, ctypes.byref(v), d_off2.data_ptr(), st2.data_ptr(), en2.data_ptr(), ctypes.byref(more), s)
    assert rc == 0 and more.value == 0
    torch.cuda.synchronize()
    m = int(full[0][-1])
    assert (st2.cpu().numpy()[:m] == full[1]).all() and (en2.cpu().numpy()[:m] == full[2]).all()
    assert (st2.cpu().numpy()[m:] == CANARY).all() and (en2.cpu().numpy()[m:] == CANARY).all()


@pytest.mark.gpu
def test_non_default_stream():
    """Everything on a fresh stream, the results read right after the calls with no synchronisation of the device."""
    import torch
    regex, cw, alphabet, plants, junk = PATTERNS[2]
    p, o = compiled(regex)
    assert_lane(p, cw)
    rng = np.random.default_rng(2)
    rows = layout_rows(rng, [ord(c) for c in alphabet], plants, n=700, max_len=120)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        check_all(p, o, rows, np.uint8, junk=[ord(c) for c in junk], kernel=False, stream=s.cuda_stream, what="stream")


ALPHABET = [ord(c) for c in "abcxyz019 AB_\n."] + [0xE9, 0x416, 0x4E2D, 0xFFFF]
EXCUSED_MODES = (3, 5, 6)  # HBM table, hot rows, compressed: these programs stay on the conversion route


def lane_or_excused(p):
    """True: the lane route at both widths.  False: conversion, excused by the program's mode.  Anything else fails."""
    ok = True
    for cw in (1, 2):
        for co in (False, True):
            r = p.find_all_packed_route(cw, co)
            if r == "conversion":
                assert p.program_info("forwards", cw, True)["mode"] in EXCUSED_MODES, ("conversion without an excuse", cw, co)
                ok = False
            else:
                assert r == "lane", r
    return ok


@pytest.mark.gpu
@pytest.mark.parametrize("seed", range(20))
def test_fuzz_patterns_without_a_transducer(seed):
    from needle_amd.pattern import PatternException
    from test_compile_vs_python_restatement import FLAG_SETS, random_regex
    rng = random.Random(9100 + seed)
    nrng = np.random.default_rng(seed)
    picked, draws = [], 0
    while len(picked) < 3:
        draws += 1
        assert draws <= 40, "no 3 patterns without a transducer in 40 draws"
        regex, flags = random_regex(rng), rng.choice(FLAG_SETS)
        try:
            p, o = compiled(regex, flags)
        except (PatternException, ValueError):
            continue
        if p.find_all_transducer(1) is None and p.find_all_transducer(2) is None:
            picked.append((p, o, (regex, flags)))
    letters = "abcdefgh"
    base = sorted({"".join(rng.choice(letters) for _ in range(rng.randint(7, 10))) for _ in range(rng.randint(3, 20))})
    words = sorted(set(base) | {w[:3] for w in base} | {w[3:-1] for w in base}, key=lambda w: (-len(w), w))
    p, o = compiled("|".join(words))
    assert p.find_all_transducer(1) is None and p.find_all_transducer(2) is None
    picked.append((p, o, ("dictionary", words[:4])))
    skipped = 0
    for p, o, what in picked:
        if not lane_or_excused(p):
            skipped += 1
            continue
        plants = words if what[0] == "dictionary" else []
        al = ALPHABET if what[0] != "dictionary" else [ord(c) for c in letters + " "]
        rows16 = layout_rows(nrng, al, plants, n=300, max_len=90, dtype=np.uint16)
        check_all(p, o, rows16, np.uint16, lead=int(nrng.integers(0, 9)), trail=int(nrng.integers(0, 2)) * 5, junk=al, kernel=False, what=what)
        al8 = [c for c in al if c < 256]
        rows8 = layout_rows(nrng, al8, plants, n=300, max_len=150)
        check_all(p, o, rows8, np.uint8, lead=int(nrng.integers(0, 9)), trail=3, junk=al8, kernel=False, what=what)
    assert skipped <= 1, "%d patterns of this seed stay on the conversion route" % skipped
