"""Capturing groups on the GPU (needle_captures_spans_packed_dev, the kernel of needle_captures_spans.h; the Python chain around it):
every case compares the planes with re.fullmatch on the clamped spans and with the CPU walk of the exported tables
(captures_cases.walk); every output has sentinels behind the list inside plane_stride and, where span_offsets[0] > 0, in front of it."""
import re

import numpy as np
import pytest

from captures_cases import (CASE_INSENSITIVE, LEFTMOST_LONGEST, MUST_WORK, SENTINEL, fuzz_patterns, fuzz_texts, re_groups, reference_planes, to_re,
                            walk)

pytestmark = pytest.mark.gpu

DASH = r"([0-9]+)-([0-9]+)"
MAIL = r"(.+)@(.+)"
CYR_CJK = "([а-яё]+) ([一-龥]+)"


@pytest.fixture(scope="module", autouse=True)
def built():
    from needle_amd import build
    build.build()


_pats = {}


def pattern(regex, flags=0):
    """(Pattern, compiled re) -- once per (regex, flags)."""
    if (regex, flags) not in _pats:
        from needle_amd.pattern import DFACompiler
        _pats[(regex, flags)] = (DFACompiler.compile(regex, "c", flags), re.compile(to_re(regex), re.IGNORECASE if flags & CASE_INSENSITIVE else 0))
    return _pats[(regex, flags)]


def device_batch(rows, cw, lead=5):
    """rows (list of str) as a packed device batch of char width `cw`: `lead` junk units in front (offsets[0] = lead), padded to 4 bytes."""
    import torch
    dt = np.uint8 if cw == 1 else np.uint16
    units = [np.frombuffer(r.encode("latin-1" if cw == 1 else "utf-16-le", "surrogatepass"), dt) for r in rows]
    junk = np.frombuffer(("1-2@3 " * (lead // 6 + 1)).encode("latin-1" if cw == 1 else "utf-16-le"), dt)[:lead]
    data = np.concatenate([junk] + units + [np.zeros(8, dt)])
    offsets = lead + np.concatenate([[0], np.cumsum([u.size for u in units])]).astype(np.int64)
    data = data[:data.size - data.size % (4 // dt().itemsize)]  # (whole 4 bytes)
    d = torch.from_numpy(data.view(np.int16) if cw == 2 else data).to("cuda")
    return d, torch.from_numpy(offsets).to("cuda")


def device_planes(p, data, offsets, spans, behind=3, stream=None):
    """The entry on a host span list -> (gstart, gend) int32[G + 1, M + behind], pre-filled with SENTINEL."""
    import torch
    off, start, end = spans
    dev = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to("cuda")
    g1 = p.group_count() + 1
    out = (torch.full((g1, len(start) + behind), SENTINEL, dtype=torch.int32, device="cuda"),
           torch.full((g1, len(start) + behind), SENTINEL, dtype=torch.int32, device="cuda"))
    got = p.captures_spans_packed(data, offsets, dev(off, np.int64), dev(start, np.int32), dev(end, np.int32), stream=stream, out=out)
    torch.cuda.synchronize()
    assert got[0] is out[0] and got[1] is out[1]
    return out[0].cpu().numpy(), out[1].cpu().numpy()


def check(regex, rows, spans, cw=1, flags=0, behind=3, lead=5, walker=True, what=""):
    p, cre = pattern(regex, flags)
    data, offsets = device_batch(rows, cw, lead)
    gs, ge = device_planes(p, data, offsets, spans, behind)
    m = len(spans[1])
    refs = [("re", lambda t: re_groups(cre, t))]
    if walker:
        tables = p.captures_tables(cw)
        refs.append(("walk", lambda t: walk(tables, t)))
    for name, fn in refs:
        ws, we = reference_planes(fn, rows, spans[0], spans[1], spans[2], p.group_count())
        for got, want, side in ((gs, ws, "start"), (ge, we, "end")):
            assert (got[:, m:] == SENTINEL).all(), (what, "columns behind the list were written")
            bad = np.argwhere(got[:, :m] != want)
            assert bad.size == 0, (what, regex, name, side, bad[:8].tolist(), [(int(got[g, k]), int(want[g, k])) for g, k in bad[:8]],
                                   [(int(spans[1][k]), int(spans[2][k])) for _, k in bad[:8]])
    return gs, ge


def spans_of(lists, front=0):
    """[[(s, e), ...] per row] -> (span_offsets int64[n + 1] starting at `front`, start, end int32 with `front` unowned entries first)."""
    off = front + np.concatenate([[0], np.cumsum([len(l) for l in lists])]).astype(np.int64)
    flat = [(0, 0)] * front + [x for l in lists for x in l]
    return off, np.array([s for s, _ in flat], np.int32), np.array([e for _, e in flat], np.int32)


def sweep(aligns, lengths, cw, lead, good, bad):
    """Rows whose spans start at every absolute alignment (in units) and have every length: per (alignment, length) a text that matches
    (good(L, k), where there is one) and one that does not (bad(L)); filler keeps the alignment; a new row every 37 spans."""
    rows, lists, row, lst = [], [], "", []
    pos = lead
    for a in aligns:
        for n in lengths:
            for text in (good(n, a), bad(n)):
                if text is None:
                    continue
                assert len(text) == n
                fill = (a - (pos + len(row))) % len(aligns)
                row += "~" * fill
                lst.append((len(row), len(row) + n))
                row += text
                if len(lst) == 37:
                    rows.append(row)
                    lists.append(lst)
                    pos += len(row)
                    row, lst = "", []
    rows.append(row)
    lists.append(lst)
    return rows, lists


def test_alignment_sweep_8bit():
    """Start alignments 0 .. 15 x lengths 0 .. 40: the dash -- where both groups' tags are set -- falls on every position of a 16-byte
    block; empty spans and spans of text that does not match (group 0 = -1)."""
    def good(n, a):
        if n < 3:
            return None
        k = 1 + (a + n) % (n - 2)
        return "7" * k + "-" + "3" * (n - k - 1)
    rows, lists = sweep(range(16), range(41), 1, 5, good, lambda n: "9" * n)
    gs, _ = check(DASH, rows, spans_of(lists), what="sweep8")
    assert (gs[0, :-3] >= 0).sum() == 16 * 38 and (gs[0, :-3] == -1).sum() == 16 * 41


def test_alignment_sweep_utf16():
    def good(n, a):
        if n < 3:
            return None
        k = 1 + (a + n) % (n - 2)
        return "ж" * k + " " + "世" * (n - k - 1)
    rows, lists = sweep(range(8), range(25), 2, 3, good, lambda n: "ё" * n)
    gs, _ = check(CYR_CJK, rows, spans_of(lists), cw=2, lead=3, what="sweep16")
    assert (gs[0, :-3] >= 0).sum() == 8 * 22


def test_slots_are_fresh_in_every_round():
    """130 matches in one row: a lane's second and third round must not see its earlier rounds' slots.  Row 0: odd matches pass
    group 2, even ones do not; row 1: the first 64 pass it, the next 64 do not, the last two do."""
    regex = r"(a)(b)?;"
    kinds = [[m % 2 == 1 for m in range(130)], [m < 64 or m >= 128 for m in range(130)]]
    rows, lists = [], []
    for kind in kinds:
        row, lst = "", []
        for k in kind:
            t = "ab;" if k else "a;"
            lst.append((len(row), len(row) + len(t)))
            row += t
        rows.append(row)
        lists.append(lst)
    gs, ge = check(regex, rows, spans_of(lists), what="rounds")
    for r, kind in enumerate(kinds):
        assert [(gs[2, r * 130 + m] >= 0) for m in range(130)] == kind


@pytest.mark.parametrize("n_rows", [1, 63, 64, 65, 130])
def test_rows_and_offsets(n_rows):
    """Row counts around the 64-row group; every third row without spans, every seventh empty; span_offsets[0] = 4 with sentinels in
    front; planes longer than the list."""
    _, cre = pattern(DASH)
    rows = ["" if r % 7 == 6 else "id%d 1%d-2 x 30-%d4;" % (r, r, r) for r in range(n_rows)]
    lists = [[] if r % 3 == 2 else [m.span() for m in cre.finditer(rows[r])] for r in range(n_rows)]
    spans = spans_of(lists, front=4)
    gs, ge = check(DASH, rows, spans, behind=5, what="rows %d" % n_rows)
    assert (gs[:, :4] == SENTINEL).all() and (ge[:, :4] == SENTINEL).all()
    assert (gs[:, 4:-5] >= 0).all()


def test_no_rows_and_no_spans():
    import torch
    p, _ = pattern(DASH)
    data, offsets = device_batch(["1-2", "3-4"], 1)
    none = torch.zeros(0, dtype=torch.int32, device="cuda")
    zero = torch.zeros(3, dtype=torch.int64, device="cuda")
    gs, ge = p.captures_spans_packed(data, offsets, zero, none, none)
    assert tuple(gs.shape) == (3, 0) and tuple(ge.shape) == (3, 0)
    gs, ge = p.captures_spans_packed(data, offsets[:1].contiguous(), zero[:1].contiguous(), none, none)  # n_rows == 0
    assert tuple(gs.shape) == (3, 0)
    off, gs, ge = p.find_all_groups_packed(data, torch.tensor([5, 5, 5], dtype=torch.int64, device="cuda"))
    assert off.tolist() == [0, 0, 0] and gs.numel() == 0


def test_malformed_lists():
    """Reversed, overlapping, repeated, negative and out-of-row spans: the result is the clamp's."""
    rng = np.random.default_rng(11)
    rows = ["12-34 5-6 x", "", "7-8", "1-2-3 44-55 6-", "9" * 30 + "-" + "1" * 30]
    lists = []
    for row in rows:
        n = len(row)
        lst = [(0, n), (0, n), (n, 0), (-5, n + 5), (n + 3, n + 9), (-9, -2), (3, 3)]
        lst += [(int(rng.integers(-3, n + 4)), int(rng.integers(-3, n + 4))) for _ in range(40)]
        for m in re.finditer(DASH, row):
            lst += [m.span(), m.span(), (m.start(), m.end() + 100)]
        lists.append(lst)
    gs, _ = check(DASH, rows, spans_of(lists), what="malformed")
    assert (gs[0] >= 0).sum() > 10 and (gs[0] == -1).sum() > 100


def test_long_spans():
    """One 9000-char span of (.+)@(.+) with many `@` (an op list per `@`), one of ([0-9]+)-([0-9]+): spans over hundreds of blocks."""
    mail = ("user%d@" * 1200 % tuple(range(1200)))[:8995] + "zzzzz"
    assert len(mail) == 9000 and mail.count("@") > 900
    gs, ge = check(MAIL, ["xx" + mail + "yy", mail], spans_of([[(2, 9002), (0, 1)], [(0, 9000), (1, 8999)]]), what="mail")
    assert (gs[1, 0], ge[1, 0], gs[2, 0], ge[2, 0]) == (2, 2 + mail.rindex("@"), 3 + mail.rindex("@"), 9002)
    num = "8" * 4499 + "-" + "5" * 4500
    gs, ge = check(DASH, [num, "ab" + num], spans_of([[(0, 9000), (0, 8000)], [(2, 9002)]]), what="digits")
    assert (ge[1, 0], gs[2, 0], gs[0, 1]) == (4499, 4500, 0)


def test_utf16_rows():
    """Chars outside the pattern's pages (Latin, Greek, a lone surrogate, U+FFFF) around and inside the spans."""
    rows = ["привет 世界", "πριν привет 世界 ￿", "привет￿世界", "￿привет 世界", "ёж 龥\ud83d", "abc 世界 привет 世"]
    lists = []
    for row in rows:
        n = len(row)
        lists.append([(0, n), (0, 9), (5, 14), (1, n), (n - 4, n), (n - 5, n - 2)] + [m.span() for m in re.finditer(CYR_CJK, row)])
    gs, _ = check(CYR_CJK, rows, spans_of(lists), cw=2, what="utf16")
    assert (gs[0] >= 0).sum() >= 6


def seeded_rows(texts, rng, n=96):
    rows = []
    for _ in range(n):
        parts = []
        for _ in range(int(rng.integers(0, 5))):
            parts.append(texts[int(rng.integers(0, len(texts)))])
            parts.append(" ;#\n"[int(rng.integers(0, 4))] * int(rng.integers(0, 3)))
        rows.append("".join(parts))
    return rows


@pytest.mark.parametrize("flags", [0, LEFTMOST_LONGEST])
@pytest.mark.parametrize("case", range(len(MUST_WORK)))
def test_language_unchanged(case, flags):
    """find_all_groups_packed's group 0 is find_all_packed's match list, match by match -- the capture program accepts exactly what the
    pattern's own automata accept -- and the groups are re.fullmatch's on every match."""
    import torch
    regex, f0, cw, texts = MUST_WORK[case]
    p, cre = pattern(regex, f0 | flags)
    rows = seeded_rows(texts, np.random.default_rng(case))
    data, offsets = device_batch(rows, cw)
    off, st, en = p.find_all_packed(data, offsets)
    off2, gs, ge = p.find_all_groups_packed(data, offsets)
    torch.cuda.synchronize()
    assert off.tolist() == off2.tolist() and st.numel() > 0
    assert gs[0].tolist() == st.tolist() and ge[0].tolist() == en.tolist()
    ws, we = reference_planes(lambda t: re_groups(cre, t), rows, off.cpu().numpy(), st.cpu().numpy(), en.cpu().numpy(), p.group_count())
    assert (gs.cpu().numpy() == ws).all() and (ge.cpu().numpy() == we).all()


def test_extract_group_and_strings():
    """extract_group_packed against slicing by re; find_all_groups_strings against re.finditer."""
    p, cre = pattern(r"(GET|POST|PUT) (/[^ ]*) HTTP/([0-9])\.([0-9])")
    rows = ["GET /a HTTP/1.1", "x POST /b/c HTTP/2.0 y PUT / HTTP/0.9", "", "HEAD / HTTP/1.1", "GET /é HTTP/1.0"] * 15
    from needle_amd.pattern import pack_strings
    data, offsets = pack_strings(rows)
    for g in (0, 1, 2, 4):
        text, toff, moff = p.extract_group_packed(data, offsets, g)
        got = [text[toff[m]:toff[m + 1]].tobytes().decode("utf-16-le") for m in range(toff.size - 1)]
        assert got == [m.group(g) for r in rows for m in cre.finditer(r)]
        assert moff.tolist() == np.concatenate([[0], np.cumsum([len(cre.findall(r)) for r in rows])]).tolist()
    p2, cre2 = pattern(r"(a(b)?)+")
    rows2 = ["aba", "xabaabx", "b", "aab ab a"]
    text, toff, _ = p2.extract_group_packed(*pack_strings(rows2), 2)  # (-1, -1) clamps to an empty row
    assert [text[toff[m]:toff[m + 1]].tobytes().decode("utf-16-le") for m in range(toff.size - 1)] == [m.group(2) or "" for r in rows2 for m in cre2.finditer(r)]
    want = [[[None if m.span(g)[0] < 0 else m.span(g) for g in range(3)] for m in cre2.finditer(r)] for r in rows2]
    assert p2.find_all_groups_strings(rows2) == want


def test_utf8_bytes():
    """find_all_groups_bytes against re on the decoded rows, the positions mapped to bytes by hand."""
    p, cre = pattern(CYR_CJK)
    strs = ["привет 世界", "abc привет 世界 ёж 龥!", "", "π привет 世", "no match", "\U0001f600ёж 龥\U0001f600"] * 9
    rows = [s.encode("utf-8") for s in strs]
    want = []
    for s in strs:
        b = lambda i: len(s[:i].encode("utf-8"))
        want.append([[(b(m.start(g)), b(m.end(g))) for g in range(3)] for m in cre.finditer(s)])
    assert p.find_all_groups_bytes(rows) == want
    assert sum(len(w) for w in want) > 30


def test_streams_and_chain():
    """A caller's stream; the chain called repeatedly without waiting for the device in between."""
    import torch
    p, cre = pattern(DASH)
    rows = ["a 1-2 b 33-44", "", "5-6"] * 40
    data, offsets = device_batch(rows, 1)
    want = [m.span(g) for r in rows for m in cre.finditer(r) for g in range(3)]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    off, gs, ge = p.find_all_groups_packed(data, offsets, stream=side.cuda_stream)
    calls = [p.find_all_groups_packed(data, offsets) for _ in range(4)]  # back to back
    side.synchronize()
    torch.cuda.synchronize()
    for o, s, e in [(off, gs, ge)] + calls:
        assert [(int(s[g, m]), int(e[g, m])) for m in range(s.size(1)) for g in range(3)] == want
    spans = spans_of([[m.span() for m in cre.finditer(r)] for r in rows])
    with torch.cuda.stream(side):
        a, b = device_planes(p, data, offsets, spans, stream=side.cuda_stream)
    assert a[:, :-3].T.reshape(-1).tolist() == [s for s, _ in want]


def test_fuzz_on_the_device():
    """The CPU fuzz's first 200 patterns, all 100 texts each as whole-row spans of one packed batch per pattern, against re.fullmatch."""
    import torch
    from needle_amd.pattern import DFACompiler
    ran = matched = 0
    for i, regex in enumerate(fuzz_patterns()[:200]):
        p = DFACompiler.compile(regex, "f")
        if not p.captures_info()["available"]:
            continue
        texts = fuzz_texts(i)
        cre = re.compile(regex)
        data, offsets = device_batch(texts, 1, lead=i % 16)
        spans = spans_of([[(0, len(t))] for t in texts])
        gs, ge = device_planes(p, data, offsets, spans, behind=1)
        ws, we = reference_planes(lambda t: re_groups(cre, t), texts, *spans, p.group_count())
        assert (gs[:, :-1] == ws).all() and (ge[:, :-1] == we).all(), regex
        assert (gs[:, -1] == SENTINEL).all()
        ran += 1
        matched += int((ws[0] >= 0).sum())
    assert ran >= 198 and matched > 1000
