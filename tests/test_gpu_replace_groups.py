"""Replace matches by templates with group references on the device (needle_replace_groups_lengths_packed_dev /
needle_replace_groups_fill_packed_dev; Pattern.splice_groups_packed, replace_all_groups_packed / replace_first_groups_packed /
replace_all_groups_strings / replace_all_groups_bytes): bit-exact against splice_groups (tests/replace_groups_cases.py) on planes that
re.fullmatch computes over the library's own match list, no tolerances.  Every device run writes into a buffer with 64 sentinel code
units in front of out_offsets[0] and 64 behind out_offsets[n]; they must come back untouched."""
import random
import re

import numpy as np
import pytest

from captures_cases import CASE_INSENSITIVE, MUST_WORK, SIXTEEN, fuzz_texts, re_groups, reference_planes, to_re
from replace_groups_cases import FUZZ_REFUSED, FUZZ_REFUSED_CAP, expand, fuzz_chosen, seeded_templates, splice_groups
from test_gpu_replace_all import check_guarded, guarded

pytestmark = pytest.mark.gpu

DASH = r"([0-9]+)-([0-9]+)"
PAIR = r"([a-c])([0-9])"
REQUEST = r"(GET|POST|PUT) (/[^ ]*) HTTP/([0-9])\.([0-9])"


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


def dt(cw):
    return np.uint8 if cw == 1 else np.uint16


def units(s, cw):
    return np.frombuffer(s.encode("latin-1" if cw == 1 else "utf-16-le", "surrogatepass"), dt(cw))


def batch(rows, cw, lead=5, trail=7):
    """rows (list of str) as a packed device batch: exactly `lead` junk units in front (offsets[0] = lead), `trail` behind, then zeros to
    whole 4 bytes.  The junk is text the patterns here match, so that a read outside the rows shows."""
    import torch
    junk = lambda k: np.resize(units("1-2 a3 [b] ", cw), k)
    parts = [junk(lead)] + [units(r, cw) for r in rows] + [junk(trail)]
    host = np.concatenate(parts)
    host = np.concatenate([host, np.zeros((-host.nbytes) % 4 // host.itemsize + 4 // host.itemsize, dt(cw))])
    offsets = lead + np.concatenate([[0], np.cumsum([p.size for p in parts[1:-1]])]).astype(np.int64)
    return torch.from_numpy(host.view(np.int16) if cw == 2 else host).to("cuda"), torch.from_numpy(offsets).to("cuda")


def library_planes(regex, rows, cw, flags=0):
    """The library's own match list of the rows with the planes re.fullmatch gives on it -> (moff int64[n + 1], gs, ge int32[G + 1, M])."""
    import torch
    p, cre = pattern(regex, flags)
    off, st, en = p.find_all_packed(*batch(rows, cw))
    torch.cuda.synchronize()
    off, st, en = off.cpu().numpy(), st.cpu().numpy(), en.cpu().numpy()
    gs, ge = reference_planes(lambda t: re_groups(cre, t), rows, off, st, en, p.group_count())
    return off, gs, ge


def expected(rows, cw, moff, gs, ge, groups, literals):
    """(the result text, its offsets from 0) by splice_groups, row by row."""
    lits = [units(x, cw) if isinstance(x, str) else np.asarray(x, dt(cw)) for x in literals]
    out = []
    for r, row in enumerate(rows):
        cols = range(int(moff[r]), int(moff[r + 1]))
        out.append(splice_groups(units(row, cw), [[(int(gs[g, m]), int(ge[g, m])) for g in range(gs.shape[0])] for m in cols], groups, lits))
    off = np.zeros(len(rows) + 1, np.int64)
    off[1:] = np.cumsum([x.size for x in out])
    return (np.concatenate(out) if out else np.zeros(0, dt(cw))).astype(dt(cw)), off


def run(rows, cw, moff, gs, ge, groups, literals, lead=5, out_start=3, want=None, stream=None, what=""):
    """splice_groups_packed of the rows and the planes into a guarded buffer against the reference (or `want`)."""
    import torch
    from needle_amd.pattern import Pattern
    text, off = expected(rows, cw, moff, gs, ge, groups, literals) if want is None else want
    data, offsets = batch(rows, cw, lead=lead)
    dev = lambda a, t: torch.from_numpy(np.ascontiguousarray(a, dtype=t)).to("cuda")
    big, out, sent = guarded(text.size, out_start, dt(cw))
    got, out_off = Pattern.splice_groups_packed(data, offsets, dev(moff, np.int64), dev(gs, np.int32), dev(ge, np.int32), groups, literals,
                                                stream=stream, out=out, out_start=out_start)
    assert got.data_ptr() == out.data_ptr()
    torch.cuda.synchronize()
    check_guarded(big, sent, text, off, out_off, out_start, dt(cw), (what, groups, "lead", lead, "out_start", out_start))
    return text, off


def case(regex, rows, cw, template, flags=0, what="", **kw):
    """The template on the library's list of the rows: the splice on re's planes, and the whole chain through the library."""
    import torch
    p, _ = pattern(regex, flags)
    moff, gs, ge = library_planes(regex, rows, cw, flags)
    groups, literals = p.parse_template(template)
    text, off = run(rows, cw, moff, gs, ge, groups, literals, what=(what, template), **kw)
    got, got_off = p.replace_all_groups_packed(*batch(rows, cw, lead=2), template)
    torch.cuda.synchronize()
    assert (got_off.cpu().numpy() == off).all() and (got.cpu().numpy().view(dt(cw)) == text).all(), (what, template, "the chain")
    return moff, gs, ge, text, off


def dash_rows(n, seed=3):
    """Rows for DASH: every seventh empty, every fifth without a match, the others with one to four matches and text around them."""
    rng = random.Random(seed)
    rows = []
    for r in range(n):
        if r % 7 == 6:
            rows.append("")
        elif r % 5 == 4:
            rows.append("no match here %d -" % r)
        else:
            rows.append("".join("%s%d-%d" % ("x" * rng.randint(0, 9), rng.randint(0, 10 ** rng.randint(1, 9)), rng.randint(0, 999)) for _ in range(rng.randint(1, 4)))
                        + " " * rng.randint(0, 3))
    return rows


@pytest.mark.parametrize("cw", [1, 2])
def test_layouts(cw):
    """Input offsets[0] in 0 .. 15 x four of the out_start in 0 .. 15 each: every alignment of the source against the output."""
    rows = dash_rows(70) if cw == 1 else [r.replace("x", "λ") for r in dash_rows(70)]
    moff, gs, ge = library_planes(DASH, rows, cw)
    assert moff[-1] > 80
    p, _ = pattern(DASH)
    groups, literals = p.parse_template("$2 <=é> $1")
    want = expected(rows, cw, moff, gs, ge, groups, literals)
    for lead in range(16):
        for k in range(4):
            run(rows, cw, moff, gs, ge, groups, literals, lead=lead, out_start=(5 * lead + 4 * k + k // 2) % 16, want=want, what="layouts")


@pytest.mark.parametrize("n_rows", [1, 63, 64, 65, 129, 200])
def test_row_counts(n_rows):
    """Row counts around the 64-row group at both widths, with empty rows and rows without matches; the whole chain too."""
    rows = dash_rows(200)[17:17 + n_rows] if n_rows < 200 else dash_rows(200)
    for cw in (1, 2):
        case(DASH, rows, cw, "$2-$1", what="rows %d" % n_rows)


def test_no_match_at_all_and_only_empty_rows():
    """A batch without any match: the planes are NULL, the rows come back as they are."""
    for cw in (1, 2):
        for rows in (["no", "", "match - here", "7-"] * 20, [""] * 70, ["x"]):
            moff, gs, ge, text, off = case(DASH, rows, cw, "$2-$1", what="no match")
            assert moff[-1] == 0 and gs.shape == (3, 0) and (text == np.concatenate([units(r, cw) for r in rows])).all()


@pytest.mark.parametrize("cw", [1, 2])
def test_identity(cw):
    """The template $0 returns the input bit for bit."""
    rows = dash_rows(130, seed=4)
    moff, gs, ge, text, off = case(DASH, rows, cw, "$0", what="identity")
    assert (text == np.concatenate([units(r, cw) for r in rows])).all() and moff[-1] > 150


@pytest.mark.parametrize("cw", [1, 2])
def test_literal_only_template_is_splice_packed(cw):
    """K = 0 goes through the new kernel and gives exactly the plain kernels' output on the same list; the empty template deletes."""
    import torch
    from needle_amd.pattern import Pattern
    rows = dash_rows(130, seed=5)
    moff, gs, ge = library_planes(DASH, rows, cw)
    data, offsets = batch(rows, cw)
    dev = lambda a, t: torch.from_numpy(np.ascontiguousarray(a, dtype=t)).to("cuda")
    for repl in ("", "#", "<n\xe9>", "0123456789abcdef" * 256):
        plain, plain_off = Pattern.splice_packed(data, offsets, dev(moff, np.int64), dev(gs[0], np.int32), dev(ge[0], np.int32), repl)
        torch.cuda.synchronize()
        want = (plain.cpu().numpy().view(dt(cw)), plain_off.cpu().numpy())
        run(rows, cw, moff, gs, ge, [], [repl], want=want, what="literal only")
        run(rows, cw, moff, gs, ge, [], [repl], what="literal only, by the definition")


@pytest.mark.parametrize("cw", [1, 2])
def test_empty_template_deletes_every_match(cw):
    rows = dash_rows(100, seed=6)
    moff, gs, ge, text, off = case(DASH, rows, cw, "", what="empty template")
    cre = re.compile(DASH)
    assert (text == np.concatenate([units(cre.sub("", r), cw) for r in rows])).all()


@pytest.mark.parametrize("cw", [1, 2])
def test_many_pieces_per_block_and_adjacent_matches(cw):
    """$2$1 on ([a-c])([0-9]): one-unit pieces back to back, up to 16 pieces in a 16-byte block at width 1; matches that touch, with no
    gap between them, and some with gaps of one unit."""
    rng = random.Random(8)
    rows = []
    for r in range(90):
        row = ""
        for _ in range(rng.randint(0, 40)):
            row += rng.choice("abc") + rng.choice("0123456789") + ("" if rng.random() < 0.8 else rng.choice(["-", "zz", "a"]))
        rows.append(row)
    for template in ("$2$1", "<$1>", "$2\\$$1$2"):
        moff, gs, ge, text, off = case(PAIR, rows, cw, template, what="pieces")
    assert moff[-1] > 1200 and int(((gs[0, 1:] == ge[0, :-1]) & (gs[0, 1:] > 0)).sum()) > 800  # adjacent matches


def test_chunk_edges():
    """The piece table's chunks: 300 matches in one row under a 3-piece template (chunks of 80 matches end inside the row, at both
    widths); 16 references between 17 non-empty literals (34 pieces a match, chunks of 7) on a row of 40 matches; a group of 65 rows in
    which only the last has matches."""
    row = "".join("%d-%d%s" % (i, 7 * i % 1000, " " * (1 + i % 3)) for i in range(300))
    for cw in (1, 2):
        moff, gs, ge, _, _ = case(DASH, ["head", row, "tail 1-2"], cw, "$2:", what="300 matches")  # pieces: $2, ":", the gap
        assert moff.tolist() == [0, 0, 300, 301]
        case(DASH, ["head", row, "tail 1-2"], cw, "$1", what="300 matches, 2 pieces")            # chunks of 120
    tmpl = "".join("%s$%d" % ("ABCDEFGHIJKLMNOPQ"[k] * (1 + k % 3), 16 - k) for k in range(16)) + "!"
    p, _ = pattern(SIXTEEN)
    groups, literals = p.parse_template(tmpl)
    assert len(groups) == 16 and all(literals)
    rows = ["..".join(["abcdefghijklmnop"] * 40) + ".", "abcdefghijklmnopabcdefghijklmnop", "abc"]
    moff, _, _, _, _ = case(SIXTEEN, rows, 1, tmpl, what="34 pieces a match")
    assert moff.tolist() == [0, 40, 42, 42]
    rows = ["row %d without" % r for r in range(64)] + ["x 1-2 y 33-44 z"]
    for cw in (1, 2):
        moff, _, _, _, _ = case(DASH, rows, cw, "$2-$1", what="only the 65th row matches")
        assert moff.tolist() == [0] * 65 + [2]


@pytest.mark.parametrize("cw", [1, 2])
def test_a_long_group_referenced_twice(cw):
    """One 5000-unit group in <$1|$1>: several wave steps through one piece, the source read twice, the output longer than the input."""
    rng = random.Random(9)
    body = "".join(rng.choice("abcdefghijklmnopqrstuvwxyz") for _ in range(5000))
    rows = ["in front [ab] ", "xy[" + body + "]z [q]", "", "behind [" + body[:700] + "]"]
    moff, gs, ge, text, off = case(r"\[([a-z]+)\]", rows, cw, "<$1|$1>", what="long group")
    assert moff.tolist() == [0, 1, 3, 3, 4] and ge[1, 1] - gs[1, 1] == 5000 and off[-1] > 11000


def test_an_unpassed_group_appends_nothing():
    rows = ["a", "b", "xaybz", "", "ab" * 50, "c"] * 12
    for cw in (1, 2):
        moff, gs, ge, text, off = case(r"(a)|(b)", rows, cw, "[$1$2]", what="unpassed")
        assert (gs[1] < 0).sum() > 500 and (gs[2] < 0).sum() > 500
    cre = re.compile(r"(a)|(b)")
    assert (text == np.concatenate([units(cre.sub(lambda m: "[" + (m.group(1) or "") + (m.group(2) or "") + "]", r), 2) for r in rows])).all()


@pytest.mark.parametrize("cw", [1, 2])
def test_kept_matches(cw):
    """Caller-made planes: plane 0 = -1 on a seeded 30 % of the matches (the other planes keep their values): those matches stay."""
    rows = dash_rows(150, seed=10) + ["1-2" * 100]
    moff, gs, ge = library_planes(DASH, rows, cw)
    rng = np.random.default_rng(10)
    kept = rng.random(gs.shape[1]) < 0.3
    gs[0, kept] = -1
    ge[0, kept & (rng.random(gs.shape[1]) < 0.5)] = -1
    assert 0.2 < kept.mean() < 0.4
    p, _ = pattern(DASH)
    for template in ("$2-$1", "<$0>", ""):
        run(rows, cw, moff, gs, ge, *p.parse_template(template), what="kept")
    gs[0, :] = -1  # every match kept: the input, bit for bit
    text, _ = run(rows, cw, moff, gs, ge, *p.parse_template("<$2>"), what="all kept")
    assert (text == np.concatenate([units(r, cw) for r in rows])).all()


@pytest.mark.parametrize("cw", [1, 2])
def test_planes_that_leave_the_row_or_are_reversed(cw):
    """The groups' planes hold anything -- outside the row, reversed, negative ends; plane 0 stays monotone but some ends lie in front
    of their starts (an empty match at the start) and the last end of a row lies behind the row: the answer is what the clamps define."""
    rows = dash_rows(140, seed=11)
    moff, gs, ge = library_planes(DASH, rows, cw)
    rng = np.random.default_rng(11)
    lens = np.repeat([len(r) for r in rows], np.diff(moff))
    m = gs.shape[1]
    for g in (1, 2):
        wild = rng.random(m) < 0.7
        gs[g, wild] = rng.integers(-3, lens[wild] + 6)
        ge[g, wild] = rng.integers(-3, lens[wild] + 6)
    gs[1, ::9], ge[1, ::9] = 0, 2 ** 31 - 1
    gs[2, ::11], ge[2, ::11] = 2 ** 31 - 1, -2 ** 31
    rev = rng.random(m) < 0.2
    ge[0, rev] = gs[0, rev] - rng.integers(0, 4, int(rev.sum()))
    last = moff[1:][np.diff(moff) > 0] - 1
    ge[0, last[::2]] = 2 ** 31 - 1
    p, _ = pattern(DASH)
    for template in ("$2-$1", "$1$1$2$0"):
        run(rows, cw, moff, gs, ge, *p.parse_template(template), what="wild planes")


def test_more_planes_than_groups():
    """n_planes > G + 1 and a plane_stride larger than the list: the planes behind the pattern's groups can be referenced too."""
    rows = dash_rows(100, seed=12)
    for cw in (1, 2):
        moff, gs, ge = library_planes(DASH, rows, cw)
        m = gs.shape[1]
        wide_s, wide_e = np.full((6, m + 9), -9, np.int32), np.full((6, m + 9), -9, np.int32)
        wide_s[:3, :m], wide_e[:3, :m] = gs, ge
        wide_s[3, :m], wide_e[3, :m] = gs[0], ge[1]   # plane 3: the match up to the dash
        wide_s[5, :m], wide_e[5, :m] = 0, 1           # plane 5: the row's first unit
        run(rows, cw, moff, wide_s, wide_e, [5, 3, 4, 2], ["", "<", ">", "", "!"], what="six planes")


def test_a_non_default_stream():
    """Lengths, cumsum and fill back to back on the caller's stream, several calls without waiting for the device in between."""
    import torch
    from needle_amd.pattern import Pattern
    rows = dash_rows(200, seed=13)
    moff, gs, ge = library_planes(DASH, rows, 1)
    p, _ = pattern(DASH)
    groups, literals = p.parse_template("$2-$1")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    want = run(rows, 1, moff, gs, ge, groups, literals, stream=side.cuda_stream, what="stream")
    data, offsets = batch(rows, 1)
    dev = lambda a, t: torch.from_numpy(np.ascontiguousarray(a, dtype=t)).to("cuda")
    args = (dev(moff, np.int64), dev(gs, np.int32), dev(ge, np.int32))
    torch.cuda.synchronize()
    calls = [Pattern.splice_groups_packed(data, offsets, *args, groups, literals, stream=side.cuda_stream) for _ in range(4)]
    chain = p.replace_all_groups_packed(data, offsets, "$2-$1", stream=side.cuda_stream)
    side.synchronize()
    for text, off in calls + [chain]:
        assert (text.cpu().numpy() == want[0]).all() and (off.cpu().numpy() == want[1]).all()


def seeded_rows(texts, rng, n):
    rows = []
    for _ in range(n):
        parts = []
        for _ in range(rng.randint(0, 4)):
            parts.append(rng.choice(texts))
            parts.append(rng.choice(" ;#\n") * rng.randint(0, 2))
        rows.append("".join(parts))
    return rows


def all_groups_template(G):
    return "<" + "|".join("$%d" % g for g in range(min(G, 15), -1, -1)) + ">" if G else "<$0$0>"


@pytest.mark.parametrize("case_no", range(len(MUST_WORK)))
def test_strings_are_re_sub(case_no):
    """replace_all_groups_strings equals re.sub with the expansion of the template on each match, on about 300 seeded rows per
    must-work pattern (leftmost-first patterns whose list is re.finditer's); replace_first_groups_packed equals count=1."""
    from needle_amd.pattern import pack_strings
    regex, flags, _, texts = MUST_WORK[case_no]
    p, cre = pattern(regex, flags)
    rows = seeded_rows(texts, random.Random(case_no), 300)
    template = all_groups_template(p.group_count())
    groups, literals = p.parse_template(template)
    repl = lambda m: expand(groups, literals, m.string, [m.span(g) for g in range(cre.groups + 1)])
    got = p.replace_all_groups_strings(rows, template)
    assert got == [cre.sub(repl, r) for r in rows]
    assert sum(g != r for g, r in zip(got, rows)) > 100
    text, off = p.replace_first_groups_packed(*pack_strings(rows), template)
    first = [text[off[i]:off[i + 1]].tobytes().decode("utf-16-le", "surrogatepass") for i in range(len(rows))]
    assert first == [cre.sub(repl, r, count=1) for r in rows]


def test_bytes_rows():
    """UTF-8 rows with 2-, 3- and 4-byte sequences; an ill-formed byte outside the matches comes back untouched."""
    regex = "([а-яё]+) ([一-龥]+)"
    p, cre = pattern(regex)
    strs = ["привет 世界", "abc привет 世界 ёж 龥!", "", "π привет 世", "no match", "\U0001f600ёж 龥\U0001f600 é"] * 9
    rows = [s.encode("utf-8") for s in strs]
    template = "$2→$1\U0001f600"
    assert p.replace_all_groups_bytes(rows, template) == [cre.sub("\\2→\\1\U0001f600", s).encode("utf-8") for s in strs]
    bad = [b"\xff " + rows[0] + b" \xc3", rows[1] + b"\x80\x80", b"\xf0\x9f" + rows[5]]
    want = [b"\xff " + cre.sub("\\2→\\1\U0001f600", strs[0]).encode() + b" \xc3", cre.sub("\\2→\\1\U0001f600", strs[1]).encode() + b"\x80\x80",
            b"\xf0\x9f" + cre.sub("\\2→\\1\U0001f600", strs[5]).encode()]
    assert p.replace_all_groups_bytes(bad, template) == want


def test_fuzz_on_the_device():
    """The first 200 patterns of the capture fuzz that have a group, three seeded templates each, the pattern's 100 texts as the rows of
    one batch: the library's list, its planes from the device, the splice against splice_groups on re.fullmatch's planes.  A pattern is
    left out only because captures_info refuses it: FUZZ_REFUSED of the 200, at most 1 %, counted without a device by
    test_replace_groups_abi.py::test_fuzz_refusals_counted_on_the_cpu."""
    import torch
    from needle_amd.pattern import DFACompiler, Pattern
    chosen = fuzz_chosen()
    assert len(chosen) == 200
    refused = ran = replaced = 0
    for i, regex in chosen:
        p = DFACompiler.compile(regex, "f")
        if not p.captures_info()["available"]:
            refused += 1
            continue
        cre, rows = re.compile(regex), fuzz_texts(i)
        data, offsets = batch(rows, 1, lead=i % 16)
        moff, dgs, dge = p.find_all_groups_packed(data, offsets)
        torch.cuda.synchronize()
        off = moff.cpu().numpy()
        gs, ge = reference_planes(lambda t: re_groups(cre, t), rows, off, dgs[0].cpu().numpy(), dge[0].cpu().numpy(), cre.groups)
        for template in seeded_templates(i, cre.groups, 3):
            groups, literals = p.parse_template(template)
            text, want_off = expected(rows, 1, off, gs, ge, groups, literals)
            big, out, sent = guarded(text.size, i % 7, np.uint8)
            _, out_off = Pattern.splice_groups_packed(data, offsets, moff, dgs, dge, groups, literals, out=out, out_start=i % 7)
            torch.cuda.synchronize()
            check_guarded(big, sent, text, want_off, out_off, i % 7, np.uint8, (regex, template))
        ran += 1
        replaced += int(off[-1])
    assert refused == FUZZ_REFUSED and refused <= FUZZ_REFUSED_CAP and ran + refused == 200 and replaced > 5000
