"""Every match of every PACKED row of big dictionaries behind the n-gram candidate filter's find-all form
(needle_amd/csrc/needle_ngram_packed.h, OP_NG_FIND_ALL; routing: packed_find_all_route in needle_api.cpp): needle_count_matches_packed_dev
and needle_find_all_csr_packed_dev of patterns that neither the transducer nor the per-lane kernel takes -- compressed, hot-rows and
HBM-table automata.  Every test first asserts Pattern.find_all_packed_filter (it fails without the route), pins the filter ON, and checks
counts and CSR against the oracle's repeated find() on every row (DFAClassBuilder.java:616-659 restated by oracle/), bit for bit against the
same calls pinned OFF (the conversion route) and against the fixed-stride find_all_csr where the rows fit one stride.

Every batch holds more than 20 matches (check_filter asserts it: `least`) except the ones that cannot by their shape -- only empty rows,
fewer than 16 bytes of text, four rows around one keyword at the tensor's end: they say so with an explicit `least` and ride along with
batches of the same pattern that do."""
import ctypes
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

from test_gpu_configs import compiled
from test_gpu_find_all_packed import check_all, flatten, oracle_all
from test_gpu_packed_dev import device_packed, layout_rows
from test_gpu_packed_prefilter import LETTERS, boundary_rows, cyr, launches, sprinkle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def enc(w, dtype=np.uint8):
    return np.array([ord(ch) for ch in w], dtype=dtype)


def nested_words(words):
    """The 1000 keywords, compounds of two of them, 5-char prefixes and inner pieces: matches inside longer live ones (no transducer)."""
    compounds = [words[i] + words[i + 1] for i in range(0, 60, 2)]
    return words + compounds + sorted({w[:5] for w in words[100:300]} | {w[1:6] for w in words[300:400]} - set(words))


@functools.lru_cache(maxsize=None)
def dictionary(kind):
    """(pattern, oracle, words), compiled once per process."""
    from needle_amd import workload as W
    latin = W.keywords(1000, min_len=6, max_len=8)
    words = {"1000": lambda: latin, "3000": lambda: W.keywords(3000, min_len=6, max_len=8), "cyr": lambda: [cyr(w) for w in latin],
             "mixed": lambda: W.keywords_mixed(300), "nested": lambda: nested_words(latin)}[kind]()
    p, o = compiled("|".join(words))
    return p, o, words


def partial_groups(rows, lists, k):
    """k rows, half of them rows with a match: more than 20 matches from 63 rows on."""
    hit = [r for r, x in zip(rows, lists) if x]
    return hit[:k // 2] + rows[300:300 + k - k // 2]


def fwd(p):
    return p.prefilter_state("forwards")["filter_launches"]


def packed_calls(p, data, offsets, stream=None):
    """count + CSR of the packed rows -> numpy (counts, offsets, start, end): three packed find-all calls (two when nothing matches)."""
    import torch
    counts = p.count_matches_packed(data, offsets, stream=stream)
    off, st, en = p.find_all_packed(data, offsets, stream=stream)
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in (counts, off, st, en)]


def check_filter(p, o, rows, dtype, lead=5, trail=7, junk=None, what="", least=21, fixed=True):
    """The packed find-all calls pinned ON against the oracle on every row, the same calls pinned OFF and (fixed) the fixed-stride and host
    entries; the forwards launch counter moves by one per call under ON and not at all under OFF.  Returns the oracle's lists."""
    cw = np.dtype(dtype).itemsize
    assert p.find_all_packed_filter(cw) and p.find_all_packed_filter(cw, count_only=True), (what, "the filter route is not available")
    assert p.find_all_packed_route(cw) == "conversion" and p.find_all_transducer(cw) is None
    lists = oracle_all(o, rows)
    want = flatten(lists)
    total = int(want[0][-1])
    assert total >= least, (what, "matches in the batch", total)
    data, offsets = device_packed(rows, dtype, lead=lead, trail=trail, junk=junk)
    p.set_prefilter(p.PREFILTER_ON)
    try:
        b = fwd(p)
        on = packed_calls(p, data, offsets)
        assert fwd(p) - b == (3 if total else 2), (what, "filter launches under ON", fwd(p) - b)
        if fixed:  # ... the fixed-stride entries on the same rows and the host entry (check_all asserts them against the oracle)
            check_all(p, o, rows, dtype, lead=lead, trail=trail, junk=junk, kernel=False, compact=False, what=what)
        p.set_prefilter(p.PREFILTER_OFF)
        b = launches(p)
        off = packed_calls(p, data, offsets)
        assert launches(p) == b, (what, "OFF launched a filter kernel")
    finally:
        p.set_prefilter(p.PREFILTER_AUTO)
    for name, g, w in zip(("counts", "offsets", "start", "end"), on, (np.diff(want[0]),) + want):
        bad = np.nonzero(g != w)[0] if g.shape == w.shape else np.array([-1])
        assert bad.size == 0, (what, name, "differs from the oracle", bad[:10], g[bad[:5]] if bad[0] >= 0 else g.shape, w[bad[:5]] if bad[0] >= 0 else w.shape)
    for name, g, w in zip(("counts", "offsets", "start", "end"), on, off):
        assert g.shape == w.shape and (g == w).all(), (what, name, "differs from the OFF route")
    return lists


# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("kind,modes", [("1000", (6,)), ("3000", (3, 5))])
def test_layouts_8bit(kind, modes):
    """1000 keywords of 6 .. 8 chars: the compressed automaton in LDS; 3000: walks out of HBM / L2.  Keyword junk before offsets[0] and
    behind offsets[n], offsets[0] = 0 and > 0, partial and whole groups, only empty rows, tiny batches, a keyword as the last row at the
    tensor's end, keywords at the rows' boundaries."""
    p, o, words = dictionary(kind)
    assert p.info()["kernel_mode"]["forwards"] in modes
    rng = np.random.default_rng(int(kind))
    junk = [ord(ch) for ch in words[0] + words[1]]
    rows = layout_rows(rng, LETTERS, words, n=1000, max_len=120)
    lists = check_filter(p, o, rows, np.uint8, lead=5, trail=7, junk=junk, what="lead 5 trail 7")
    check_filter(p, o, rows, np.uint8, lead=0, trail=0, junk=junk, what="offsets[0] = 0, last row at the tensor's end")
    check_filter(p, o, rows, np.uint8, lead=133, trail=0, junk=junk, what="offsets[0] > 0, last row at the tensor's end")
    one = np.concatenate([np.concatenate([enc(words[30 + k]), np.full(k % 3, 32, np.uint8)]) for k in range(25)])   # n_rows 1: 25 keywords
    check_filter(p, o, [one], np.uint8, lead=3, trail=5, junk=junk, what="n_rows 1")
    for k in (63, 64, 65, 130):
        check_filter(p, o, partial_groups(rows, lists, k), np.uint8, lead=3, trail=5, junk=junk, what="n_rows %d" % k)
    check_filter(p, o, [np.zeros(0, np.uint8)] * 70, np.uint8, lead=9, trail=9, junk=junk, what="only empty rows", least=0)
    w = enc(words[2])
    for tiny in ([w[:15]], [w], [np.zeros(0, np.uint8), w[:6], np.zeros(0, np.uint8), w[:1]], [w[:3], w[3:6]]):  # under 16 bytes in all
        assert sum(r.size for r in tiny) < 16
        check_filter(p, o, tiny, np.uint8, lead=0, trail=0, junk=junk, what="tiny batch, nothing around it", least=0)
        check_filter(p, o, tiny, np.uint8, lead=21, trail=30, junk=junk, what="tiny batch inside keyword junk", least=0)
    wl = enc(words[4])
    for k in (70, 3):  # a keyword as the batch's last row: it starts inside the batch's last 16 chars
        head = partial_groups(rows, lists, k)
        got = check_filter(p, o, head + [wl], np.uint8, lead=0, trail=0, junk=junk, what="keyword is the last row, tensor's end", least=21 if k == 70 else 1)
        assert got[-1] == [(0, wl.size)]
        check_filter(p, o, head + [wl, w[:2]], np.uint8, lead=2, trail=9, junk=junk, what="keyword in the batch's last 16 chars", least=21 if k == 70 else 1)
    b = boundary_rows(rng, words, LETTERS, np.uint8)
    check_filter(p, o, b, np.uint8, lead=7, trail=2, junk=junk, what="boundaries", least=100)
    check_filter(p, o, b[::-1], np.uint8, lead=0, trail=0, junk=junk, what="boundaries, reversed", least=100)


def group_end_rows(rng, words, warm):
    """Rows for the paths of the group's end, by kind: (rows, kinds).  back: two keywords back to back; near: two keywords fewer than `warm`
    chars apart; overlap: a keyword that begins inside the previous match's tail; many: 3 .. 40 keywords."""
    al = np.array(LETTERS[:-1], dtype=np.uint8)
    fill = lambda k: np.full(int(k), 32, np.uint8) if k < 3 else np.concatenate([[32], rng.choice(al, int(k) - 2), [32]]).astype(np.uint8)
    pick = lambda: enc(words[int(rng.integers(0, len(words)))])
    heads = {}
    for w in words:
        heads.setdefault(w[:2], w)
    pairs = [(a, heads[a[-2:]]) for a in words if a[-2:] in heads and heads[a[-2:]] != a]
    assert len(pairs) > 20
    rows, kinds = [], []
    for i in range(640):
        kind = ("back", "near", "overlap", "many", "plain")[i % 5]
        if kind == "back":
            r = np.concatenate([fill(rng.integers(0, 30)), pick(), pick(), fill(rng.integers(0, 30))])
        elif kind == "near":
            r = np.concatenate([fill(rng.integers(0, 30)), pick(), fill(rng.integers(1, warm)), pick(), fill(rng.integers(0, 30))])
        elif kind == "overlap":
            a, b = pairs[int(rng.integers(0, len(pairs)))]
            r = np.concatenate([fill(rng.integers(0, 30)), enc(a), enc(b)[2:], fill(rng.integers(3, 30))])
        elif kind == "many":
            parts = []
            for _ in range(3 + (i // 5) % 38):
                parts += [pick(), fill(rng.integers(0, 12))]
            r = np.concatenate([fill(rng.integers(0, 9))] + parts)
        else:
            r = rng.choice(np.array(LETTERS, dtype=np.uint8), int(rng.integers(0, 120))).astype(np.uint8)
        rows.append(r.astype(np.uint8))
        kinds.append(kind)
    return rows, kinds


def assert_group_end_paths(lists, kinds, warm):
    """The oracle's answers show that the rows are what their kind says (none of the paths is vacuous)."""
    by = lambda k: [x for x, kk in zip(lists, kinds) if kk == k]
    assert sum(1 for x in by("back") if len(x) >= 2 and x[0][1] == x[1][0]) > 100
    assert sum(1 for x in by("near") if len(x) >= 2 and 0 < x[1][0] - x[0][1] < warm) > 100
    assert sum(1 for x in by("overlap") if len(x) == 1) > 60        # the second keyword is in the text and is skipped
    many = [len(x) for x in by("many")]
    assert min(many) >= 3 and max(many) >= 40 and len(set(many)) > 20


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["1000", "3000"])
def test_paths_of_the_groups_end(kind):
    """Back-to-back keywords and keywords fewer than `warm` chars apart (the window is run again from the cursor), a keyword overlapping the
    previous match's tail (skipped, as the reference skips it), rows with 3 .. 40 keywords (more candidates than slots: the match-by-match
    loop)."""
    p, o, words = dictionary(kind)
    assert p.find_all_packed_filter(1)
    warm = p.prefilter_info("forwards")["warm"]
    assert warm >= 4
    rng = np.random.default_rng(5 + int(kind))
    rows, kinds = group_end_rows(rng, words, warm)
    lists = check_filter(p, o, rows, np.uint8, lead=5, trail=7, junk=[ord(c) for c in words[0]], what="group-end paths")
    assert_group_end_paths(lists, kinds, warm)
    order = rng.permutation(len(rows))
    check_filter(p, o, [rows[i] for i in order], np.uint8, lead=0, trail=0, junk=[ord(c) for c in words[0]], what="group-end paths, shuffled")


@pytest.mark.gpu
def test_nested_dictionary_every_lead():
    """A big nested dictionary -- the 1000 keywords, compounds of two of them, 5-char prefixes and inner pieces -- has no transducer; on
    cut compounds (`international|inter|nation` on "internationa ": a run crosses a match that ends before its window) the rows fall to the
    re-run and the match-by-match loop.  Every lead 0 .. 15 of the stream."""
    p, o, words = dictionary("nested")
    assert p.find_all_transducer(1) is None and p.find_all_packed_filter(1)
    texts = [np.resize(enc(words[1000 + k][:-1] + " "), 3000) for k in range(3)]   # compound k = keyword 2k + keyword 2k + 1, cut by one char
    rng = np.random.default_rng(8)
    short = layout_rows(rng, LETTERS, words[:1000] + words[1030:], n=130, max_len=100)
    for lead in range(16):
        rows = [texts[0], texts[1][:77], texts[2]] + (short if lead % 5 == 0 else short[:20])
        lists = check_filter(p, o, rows, np.uint8, lead=lead, trail=4, junk=[ord(c) for c in words[1000]], what="lead %d" % lead)
        assert len(lists[0]) > 100 and lists[0][0] == (0, len(words[0]))   # the compound's first keyword, again and again


def long_batch(words):
    """About 2000 short rows, one row of 70 000 and one of 200 000 chars; the long rows carry, beyond position 65 535, a back-to-back pair,
    an overlapping pair and a stretch with more than two candidates, and single keywords before, across and far beyond it."""
    rng = np.random.default_rng(17)
    al = np.array(LETTERS, dtype=np.uint8)
    heads = {}
    for w in words:
        heads.setdefault(w[:2], w)
    a = next(w for w in words if w[-2:] in heads and heads[w[-2:]] != w)
    b = heads[a[-2:]]

    def long_row(n):
        r = rng.choice(al, n).astype(np.uint8)
        at = {}

        def put(name, pos, text):
            r[pos - 1] = r[pos + len(text)] = 32
            r[pos:pos + len(text)] = enc(text)
            at[name] = pos
        put("before", 1000, words[5])
        put("straddle", 65535 - 3, words[7])
        put("back", 65536 + 300, words[8] + words[9])
        put("overlap", 65536 + 700, a + b[2:])
        put("stretch", 65536 + 1100, " ".join(words[10:16]))
        put("far", n - 2000, words[16])
        put("end", n - len(words[17]) - 1, words[17])
        return r, at
    short = layout_rows(rng, LETTERS, words, n=2000, max_len=60)
    l70, at70 = long_row(70000)
    l200, at200 = long_row(200000)
    rows = list(short)
    rows.insert(777, l70)
    rows.insert(1411, l200)
    return rows, (777, at70), (1411, at200), (a, b)


def assert_long_rows(lists, words, i70, i200, ab):
    a, b = ab
    for idx, at in (i70, i200):
        m = lists[idx]
        assert sum(1 for s, e in m if s > 65535) >= 10
        assert (at["before"], at["before"] + len(words[5])) in m and (at["straddle"], at["straddle"] + len(words[7])) in m
        k = m.index((at["back"], at["back"] + len(words[8])))
        assert m[k + 1] == (at["back"] + len(words[8]), at["back"] + len(words[8]) + len(words[9]))       # back to back beyond 65 535
        k = m.index((at["overlap"], at["overlap"] + len(a)))
        assert m[k + 1][0] >= at["overlap"] + len(a) + len(b) - 2                                          # the overlapping keyword is skipped
        k = m.index((at["stretch"], at["stretch"] + len(words[10])))
        assert [e - s for s, e in m[k:k + 6]] == [len(w) for w in words[10:16]]                            # more than two candidates in a row
        assert (at["far"], at["far"] + len(words[16])) in m and m[-1] == (at["end"], at["end"] + len(words[17]))


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["1000", "3000"])
def test_long_rows(kind):
    """Rows of 70 000 and 200 000 chars among 2000 short ones: window ends, cursors and positions are 32 bits throughout."""
    p, o, words = dictionary(kind)
    rows, i70, i200, ab = long_batch(words)
    lists = check_filter(p, o, rows, np.uint8, lead=13, trail=9, junk=[ord(c) for c in words[0]], what="long among short", fixed=False)
    assert_long_rows(lists, words, i70, i200, ab)


DIRECT_CHILD = r'''
import sys
sys.path.insert(0, "."); sys.path.insert(0, "tests")
import numpy as np
import test_gpu_find_all_packed_filter as T
for kind in ("1000", "3000"):
    p, o, words = T.dictionary(kind)
    rows, i70, i200, ab = T.long_batch(words)
    lists = T.check_filter(p, o, rows, np.uint8, lead=13, trail=9, junk=[ord(c) for c in words[0]], what="direct groups among filtered ones", fixed=False)
    T.assert_long_rows(lists, words, i70, i200, ab)
p, o, words = T.dictionary("cyr")
rng = np.random.default_rng(3)
al = [0x0430 + k for k in range(26)] + [32]
rows = T.sprinkle(T.layout_rows(rng, al, words, n=600, max_len=150, dtype=np.uint16), rng)
T.check_filter(p, o, rows, np.uint16, lead=1, trail=0, junk=[ord(c) for c in words[0]], what="direct groups, 16-bit")
print("DIRECT-CHILD-OK")
'''


@pytest.mark.gpu
def test_long_rows_direct_groups():
    """The same batch with NEEDLE_PACKED_DIRECT_ABOVE=2000 (read once per process: a child): groups whose span exceeds 2000 chars see no
    filter -- every row is searched match by match from char 0 -- among groups that are filtered."""
    r = subprocess.run([sys.executable, "-c", DIRECT_CHILD], env=dict(os.environ, NEEDLE_PACKED_DIRECT_ABOVE="2000"), capture_output=True, text=True,
                       timeout=900, cwd=ROOT)
    assert "DIRECT-CHILD-OK" in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["cyrillic", "latin", "mixed"])
def test_utf16(which):
    """UTF-16 rows: the Cyrillic one-page dictionary with other-page chars sprinkled in (the page's byte program, narrowed on load), the
    Latin dictionary over UTF-16 rows (page 0), the mixed-script dictionary (the WIDE filter)."""
    rng = np.random.default_rng(len(which))
    if which == "mixed":
        from needle_amd import workload as W
        p, o, words = dictionary("mixed")
        assert p.utf16_route() is None
        host = W.mixed_keyword_batch(np, words, 4000, 1500, 152)
        lens = rng.integers(0, 151, 1500)
        lens[:48] = np.arange(48)
        lens[200:264] = 0
        rows = [host[i, :lens[i]].astype(np.uint16) for i in range(1500)]
        for i in range(0, 1500, 9):      # keywords of every script at both ends of rows
            rows[i] = np.concatenate([enc(words[(i * 5) % len(words)], np.uint16), rows[i][:100], enc(words[(i * 7 + 1) % len(words)], np.uint16)])
        al = [ord(c) for w in words[:40] for c in w] + [32]
    else:
        p, o, words = dictionary("cyr" if which == "cyrillic" else "1000")
        assert p.utf16_route() is not None and p.utf16_route()[0] == (4 if which == "cyrillic" else 0)
        al = ([0x0430 + k for k in range(26)] + [32]) if which == "cyrillic" else LETTERS
        rows = sprinkle(layout_rows(rng, al, words, n=1500, max_len=150, dtype=np.uint16), rng)
    junk = [ord(ch) for ch in words[0] + words[1]]
    lists = check_filter(p, o, rows, np.uint16, lead=5, trail=7, junk=junk, what=which)
    check_filter(p, o, rows, np.uint16, lead=0, trail=0, junk=junk, what=which + ", tensor's ends")
    one = np.concatenate([np.concatenate([enc(words[30 + k], np.uint16), np.full(k % 3, 32, np.uint16)]) for k in range(25)])
    check_filter(p, o, [one], np.uint16, lead=3, trail=5, junk=junk, what=which + " n_rows 1")
    for k in (64, 65, 130):
        check_filter(p, o, partial_groups(rows, lists, k), np.uint16, lead=3, trail=5, junk=junk, what="%s n_rows %d" % (which, k))
    b = boundary_rows(rng, words, al, np.uint16)
    check_filter(p, o, sprinkle(b, rng) if which != "mixed" else b, np.uint16, lead=1, trail=0, junk=junk, what=which + " boundaries")
    check_filter(p, o, [enc(words[3][:7], np.uint16)], np.uint16, lead=0, trail=0, junk=junk, what=which + " tiny", least=0)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["1000", "3000"])
def test_capacity_more_and_canary(kind):
    """Offsets with room for one match per row: more = 1, every row's first match filed, nothing written behind the offsets' total; exact
    room: more = 0; the counting pass gives the CSR row sizes."""
    import torch
    from needle_amd import _lib
    p, o, words = dictionary(kind)
    assert p.find_all_packed_filter(1)
    rng = np.random.default_rng(12)
    rows, _ = group_end_rows(rng, words, 8)
    want = oracle_all(o, rows)
    counts = np.array([len(x) for x in want])
    assert (counts > 1).sum() > 300 and counts.sum() > 20
    data, offsets = device_packed(rows, np.uint8, lead=5, trail=7, junk=[ord(c) for c in words[0]])
    v = p._packed_dev_view(data, offsets)
    s = torch.cuda.current_stream().cuda_stream
    CANARY = -1234567
    p.set_prefilter(p.PREFILTER_ON)
    try:
        for room, expect_more in ((np.minimum(counts, 1), 1), (counts, 0)):
            off = np.zeros(len(rows) + 1, np.int64)
            off[1:] = np.cumsum(room)
            total = int(off[-1])
            st = torch.full((total + 64,), CANARY, dtype=torch.int32, device="cuda")
            en = torch.full((total + 64,), CANARY, dtype=torch.int32, device="cuda")
            d_off = torch.from_numpy(off).to("cuda")
            more = ctypes.c_int(7)
            b = fwd(p)
            rc = _lib.lib().needle_find_all_csr_packed_dev(p._h, ctypes.byref(v), d_off.data_ptr(), st.data_ptr(), en.data_ptr(), ctypes.byref(more), s)
            assert rc == 0 and more.value == expect_more and fwd(p) - b == 1
            torch.cuda.synchronize()
            hs, he = st.cpu().numpy(), en.cpu().numpy()
            filed = [m for x, k in zip(want, room) for m in x[:k]]
            assert hs[:total].tolist() == [a for a, _ in filed] and he[:total].tolist() == [b_ for _, b_ in filed]
            assert (hs[total:] == CANARY).all() and (he[total:] == CANARY).all()
        b = fwd(p)
        got = p.count_matches_packed(data, offsets)
        torch.cuda.synchronize()
        assert fwd(p) - b == 1 and (got.cpu().numpy() == counts).all()
    finally:
        p.set_prefilter(p.PREFILTER_AUTO)


def chunked_batch(words):
    """300 short rows, one row of 60 000 chars, 300 short rows: the conversion route splits it into several chunks."""
    rng = np.random.default_rng(23)
    short = layout_rows(rng, LETTERS, words, n=600, max_len=120)
    long_row = rng.choice(np.array(LETTERS, dtype=np.uint8), 60000).astype(np.uint8)
    for k in range(40):
        w = enc(words[20 + k])
        long_row[1000 + 1400 * k:1000 + 1400 * k + w.size] = w
    return short[:300] + [long_row] + short[300:]


SWITCH_CHILD = r'''
import sys
sys.path.insert(0, "."); sys.path.insert(0, "tests")
import numpy as np
import test_gpu_find_all_packed_filter as T
p, o, words = T.dictionary("1000")
assert not p.find_all_packed_filter(1) and not p.find_all_packed_filter(2, count_only=True)   # the query obeys the switch as the routing does
assert p.find_all_packed_route(1) == "conversion"
rows = T.chunked_batch(words)
want = T.flatten(T.oracle_all(o, rows))
data, offsets = T.device_packed(rows, np.uint8, 5, 7, [ord(c) for c in words[0]])
moved = []
for mode in (p.PREFILTER_ON, p.PREFILTER_AUTO, p.PREFILTER_OFF):
    p.set_prefilter(mode)
    b = T.fwd(p)
    counts, off, st, en = T.packed_calls(p, data, offsets)
    moved.append(T.fwd(p) - b)
    assert (counts == np.diff(want[0])).all() and (off == want[0]).all() and (st == want[1]).all() and (en == want[2]).all(), mode
assert want[0][-1] > 20 and moved[2] == 0
print("SWITCH-CHILD-OK launches under ON / AUTO / OFF for three calls:", moved)
'''


@pytest.mark.gpu
def test_which_kernel_ran():
    """filter_launches (forwards) rises by exactly one per packed find-all call under ON, on a batch that the conversion route splits into
    three chunks (300 short rows, one row of 60 000 chars, 300 short rows); AUTO on this quiet text does the same, OFF launches none.  With
    NEEDLE_PREFILTER_PACKED=0 or NEEDLE_FIND_ALL_FILTER_PACKED=0 (children) the query says no and the answers are the same.

    The conversion route of the commit before this one converts the batch in three chunks -- the first 300 rows, the long row with the few
    rows behind it that still fit its stride, the rest -- and the first and the last of them have the fixed-stride filter's shape: it
    moves the counter by 2 per call, not 1, so this assertion discriminates beside the find_all_packed_filter one.  (Derived from the
    chunking rule of packed_find_all_by_conversion and ngram_shape_ok; the NEEDLE_FIND_ALL_FILTER_PACKED=0 child prints what that route
    gives in this build.)"""
    import torch
    p, o, words = dictionary("1000")
    assert p.find_all_packed_filter(1)
    rows = chunked_batch(words)
    want = flatten(oracle_all(o, rows))
    assert want[0][-1] > 20 and len(oracle_all(o, [rows[300]])[0]) >= 40
    data, offsets = device_packed(rows, np.uint8, 5, 7, [ord(c) for c in words[0]])
    results = {}
    for mode, per_call in ((p.PREFILTER_ON, 1), (p.PREFILTER_AUTO, 1), (p.PREFILTER_OFF, 0)):
        p.set_prefilter(mode)
        for _ in range(2):
            b = fwd(p)
            counts = p.count_matches_packed(data, offsets)
            torch.cuda.synchronize()
            assert fwd(p) - b == per_call, (mode, "count_matches_packed", fwd(p) - b)
            b = fwd(p)
            off, st, en = p.find_all_packed(data, offsets)
            torch.cuda.synchronize()
            assert fwd(p) - b == 2 * per_call, (mode, "find_all_packed (count + fill)", fwd(p) - b)
        results[mode] = [t.cpu().numpy() for t in (counts, off, st, en)]
        assert (results[mode][0] == np.diff(want[0])).all() and all((g == w).all() for g, w in zip(results[mode][1:], want)), mode
    p.set_prefilter(p.PREFILTER_AUTO)
    for env in ({"NEEDLE_PREFILTER_PACKED": "0"}, {"NEEDLE_FIND_ALL_FILTER_PACKED": "0"}):
        r = subprocess.run([sys.executable, "-c", SWITCH_CHILD], env=dict(os.environ, **env), capture_output=True, text=True, timeout=900, cwd=ROOT)
        assert "SWITCH-CHILD-OK" in r.stdout, (env, r.stdout[-2000:] + r.stderr[-3000:])


@pytest.mark.gpu
def test_flood_watch_suspends_the_route():
    """Flood text (tests/test_gpu_prefilter_watch.py) under AUTO: the first packed find-all call takes the filter kernel, the next one
    evaluates it, finds more than 16 candidates per KiB and suspends the route -- that call and the following ones go by conversion (whose
    fixed-stride calls obey the same suspension); the answers are the oracle's in every state; ON is never suspended."""
    import torch
    _, _, words = dictionary("1000")
    p, o = compiled("|".join(words))             # (a pattern of its own: the watch's counters and its suspension are per pattern)
    assert p.find_all_packed_filter(1)
    n, stride = 64 * 100 + 9, 256
    rng = np.random.default_rng(5)
    long_words = [w for w in words if len(w) >= 6][:512]
    wt8 = np.full((len(long_words), 8), 32, dtype=np.uint8)
    for i, w in enumerate(long_words):
        t = enc(w[-8:])
        t[0] = ord("q") if t[0] != ord("q") else ord("z")
        wt8[i, 8 - t.size:] = t
    flood = wt8[rng.integers(0, len(long_words), (n, stride // 8))].reshape(n, stride).copy()
    flood[::5, 8:8 + len(words[0])] = enc(words[0])
    lens = rng.integers(150, stride + 1, n)
    assert lens.sum() > (1100 << 10)         # every call gives the watch more than the 1024 KiB it evaluates on
    rows = [flood[i, :lens[i]] for i in range(n)]
    want = np.array([len(x) for x in oracle_all(o, rows)])
    assert want.sum() > 20
    data, offsets = device_packed(rows, np.uint8, 3, 5, None)

    def call():
        got = p.count_matches_packed(data, offsets)
        torch.cuda.synchronize()
        assert (got.cpu().numpy() == want).all()

    st = p.prefilter_state("forwards")
    assert st["mode"] == p.PREFILTER_AUTO and st["suspended_calls_left"] == 0
    b = st["filter_launches"]
    call()                                       # the filter kernel; its counters arrive behind it
    st = p.prefilter_state("forwards")
    assert st["filter_launches"] == b + 1 and st["suspended_calls_left"] == 0, st
    call()                                       # evaluates the first launch: flooded -> conversion, now and for the calls that follow
    st = p.prefilter_state("forwards")
    assert st["last_candidates_per_kib"] > 16 and st["suspended_calls_left"] > 0 and st["filter_launches"] == b + 1, st
    call()
    assert p.prefilter_state("forwards")["filter_launches"] == b + 1
    p.set_prefilter(p.PREFILTER_ON)              # pinned ON: the filter kernel every time
    try:
        for _ in range(2):
            call()
        assert p.prefilter_state("forwards")["filter_launches"] == b + 3
    finally:
        p.set_prefilter(p.PREFILTER_AUTO)


@pytest.mark.gpu
def test_non_default_stream():
    """A non-default stream, the results read right behind the calls on that stream."""
    import torch
    p, o, words = dictionary("1000")
    assert p.find_all_packed_filter(1)
    rng = np.random.default_rng(31)
    rows = layout_rows(rng, LETTERS, words, n=3000, max_len=300)
    want = flatten(oracle_all(o, rows))
    assert want[0][-1] > 20
    p.set_prefilter(p.PREFILTER_ON)
    try:
        s = torch.cuda.Stream()
        b = fwd(p)
        with torch.cuda.stream(s):
            data, offsets = device_packed(rows, np.uint8, 3, 3, [ord(c) for c in words[0]])
            counts = p.count_matches_packed(data, offsets, stream=s.cuda_stream)
            off, st, en = p.find_all_packed(data, offsets, stream=s.cuda_stream)
            got = [t.to("cpu", non_blocking=False).numpy() for t in (counts, off, st, en)]   # (copies on s: ordered behind the kernels)
        assert fwd(p) - b == 3
        assert (got[0] == np.diff(want[0])).all() and all((g == w).all() for g, w in zip(got[1:], want))
    finally:
        p.set_prefilter(p.PREFILTER_AUTO)


FUZZ_CHILD = r'''
import sys, random
sys.path.insert(0, "."); sys.path.insert(0, "tests")
import numpy as np
import test_gpu_find_all_packed_filter as T
seed = int(sys.argv[1])
rng = random.Random(9000 + seed)
nrng = np.random.default_rng(seed)
letters = "abcdefgh"
redrawn = 0
while True:   # a dictionary that another route takes, or one without a filter, is redrawn, not skipped
    words = sorted({"".join(rng.choice(letters) for _ in range(rng.randint(5, 9))) for _ in range(rng.randint(5, 60))})
    words += sorted({rng.choice(words) + rng.choice(words) + rng.choice(letters) for _ in range(rng.randint(1, 6))})   # compounds one char longer
    rng.shuffle(words)
    p, o = T.compiled("|".join(words))
    if p.find_all_packed_filter(1) and p.find_all_packed_filter(2):
        break
    redrawn += 1
    assert redrawn < 50
al = [ord(ch) for ch in letters + " "]
junk = [ord(ch) for ch in words[0]]
rows = T.layout_rows(nrng, al, words, n=1500, max_len=200)
T.check_filter(p, o, rows, np.uint8, lead=int(nrng.integers(0, 9)), trail=3, junk=junk, what=("dictionary", seed, words[:5]))
rows16 = T.sprinkle(T.layout_rows(nrng, al, words, n=1500, max_len=200, dtype=np.uint16), nrng)
T.check_filter(p, o, rows16, np.uint16, lead=int(nrng.integers(0, 9)), trail=int(nrng.integers(0, 2)) * 5, junk=junk, what=("dictionary 16-bit", seed, words[:5]))
T.check_filter(p, o, T.boundary_rows(nrng, words, al, np.uint8), np.uint8, lead=int(nrng.integers(0, 17)), trail=0, junk=junk, what=("boundaries", seed))
print("FUZZ-CHILD-OK", redrawn)
'''


@pytest.mark.gpu
@pytest.mark.parametrize("seed", range(6))
def test_fuzz_random_dictionaries(seed):
    """Seeded random nested dictionaries (words of 5 .. 9 chars and a few compounds of two of them and one more char: the second word
    matches while the compound is still live, which leaves most draws a transducer all the same and about a quarter of them none; the rest
    are redrawn) over random packed batches, 8- and 16-bit, at NEEDLE_PREFILTER=2 so that small automata carry a filter, with the per-lane
    route switched off so that they reach this one (both read once per process: a child)."""
    env = dict(os.environ, NEEDLE_PREFILTER="2", NEEDLE_PAIR_MAX_BYTES="0", NEEDLE_PACKED_FIND_ALL_LANE="0")
    r = subprocess.run([sys.executable, "-c", FUZZ_CHILD, str(seed)], env=env, capture_output=True, text=True, timeout=900, cwd=ROOT)
    assert "FUZZ-CHILD-OK" in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]
