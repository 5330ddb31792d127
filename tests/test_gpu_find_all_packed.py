"""Every match of every packed row (needle_count_matches_packed_dev / needle_find_all_csr_packed_dev /
needle_find_all_compact16_packed_dev / needle_find_all_csr_packed_host): bit-exact against the oracle's repeated find() on each
row (oracle/walker.py find_all) and against rows_from_packed + the fixed-stride entries on the same rows -- counts, starts,
ends, `more`.  Patterns through both routes (the packed find-all kernel: keyword unions on the lengths transducer, runs on the
RUN transducer; the conversion route: nullable patterns, backward walks, nested dictionaries), 8- and 16-bit layouts with
edge cases, the result forms, a non-default stream, 10^7 ragged rows and a seeded fuzz."""
import random

import numpy as np
import pytest

from test_gpu_configs import compiled
from test_gpu_packed_dev import device_packed, layout_rows


def oracle_all(o, rows):
    return [o.find_all(np.asarray(r), limit=1 << 30) for r in rows]


def flatten(lists):
    off = np.zeros(len(lists) + 1, np.int64)
    off[1:] = np.cumsum([len(x) for x in lists])
    st = np.array([s for x in lists for s, _ in x], np.int32)
    en = np.array([e for x in lists for _, e in x], np.int32)
    return off, st, en


def check_all(p, o, rows, dtype, lead=5, trail=7, junk=None, kernel=None, compact=True, stream=None, what=""):
    """Counts / CSR (device and host) / compact16 of the packed rows against the oracle and the fixed-stride entries."""
    import torch
    from needle_amd.pattern import Pattern
    cw = np.dtype(dtype).itemsize
    if kernel is not None:
        assert (p.find_all_transducer(cw) is not None) == kernel, ("route", what)
    data, offsets = device_packed(rows, dtype, lead=lead, trail=trail, junk=junk)
    want = flatten(oracle_all(o, rows))
    counts = p.count_matches_packed(data, offsets, stream=stream)
    off, st, en = p.find_all_packed(data, offsets, stream=stream)
    if stream is None:
        torch.cuda.synchronize()
    assert (counts.cpu().numpy() == np.diff(want[0])).all(), ("counts", what)
    assert (off.cpu().numpy() == want[0]).all(), ("offsets", what)
    assert (st.cpu().numpy() == want[1]).all() and (en.cpu().numpy() == want[2]).all(), ("start/end", what)
    # the same rows at a fixed stride through the fixed-stride entries
    frows, flens, _ = Pattern.rows_from_packed(data, offsets)
    xo, xs, xe = p.find_all_csr(frows, flens)
    assert torch.equal(xo, off) and torch.equal(xs, st) and torch.equal(xe, en), ("fixed-stride", what)
    # the host entry on the same packed rows
    h = data.cpu().numpy().view(dtype)
    ho, hs, he = p.find_all_packed(h, offsets.cpu().numpy())
    assert (ho == want[0]).all() and (hs == want[1]).all() and (he == want[2]).all(), ("host", what)
    longest = max([len(r) for r in rows] + [0])
    if compact and p.find_all_transducer(cw) is not None and longest <= 65535:
        for mpr in (32, 2):
            co, cse, cm = p.find_all_compact16_packed(data, offsets, max_per_row=mpr, stream=stream)
            fo, fse, fm = p.find_all_compact16(frows, max_per_row=mpr, lengths=flens)
            torch.cuda.synchronize()
            assert torch.equal(co, fo) and torch.equal(cse, fse) and cm == fm, ("compact16", mpr, what)
            if mpr == 32 and not cm:
                se = cse.cpu().numpy().view(np.uint32)
                assert (co.cpu().numpy() == want[0]).all() and ((se & 0xFFFF) == want[1]).all() and ((se >> 16) == want[2]).all(), what
    return want


PATTERNS = [
    # (regex, char width, alphabet, planted words, junk, takes the packed find-all kernel)
    ("Sherlock|Holmes|Watson|Irene|Adler|John|Baker", 1, "SherlockHmsWatnIdJB ", ["Sherlock", "Holmes", "Baker"], "Holmes", True),
    ("[0-9]+", 1, "abcxyz 0123456789", [], "0123", True),
    ("[a-z]{3}[a-z]*", 1, "abc xyz0", [], "abcd", True),
    ("a.c", 1, "abcx\n", ["abc", "axc"], "abc", True),
    ("[α-ω]{2}[α-ω]*", 2, "ab αβω￿", ["αβγ"], "αβγ", True),
    ("Жук|ЖЗ|中文字", 2, "ЖукЗ中文字 a", ["Жук", "中文字"], "ЖЗ", True),
    ("[a-c]*", 1, "abcd", [], "abc", False),                                     # nullable
    ("international|inter|nation", 1, "interntiol ", ["international", "inter", "nation"], "inter", False),
    ("http://.+", 1, "htp:/abc.x\n", ["http://", "http://a.b"], "http://x", False),  # backward walks
    ("[a-z一-丠]+[0-9]|ЖЗ+", 2, "az9一丐丰ЖЗ ", ["一丁x7", "ЖЗЗ"], "一a1", False),
]


@pytest.mark.gpu
@pytest.mark.parametrize("regex,cw,alphabet,plants,junk,kernel", PATTERNS)
def test_patterns_and_layouts(regex, cw, alphabet, plants, junk, kernel):
    p, o = compiled(regex)
    dtype = np.uint8 if cw == 1 else np.uint16
    rng = np.random.default_rng(11 + len(regex))
    al = [ord(ch) for ch in alphabet]
    jk = [ord(ch) for ch in junk]
    rows = layout_rows(rng, al, plants, n=700, max_len=120, dtype=dtype)
    check_all(p, o, rows, dtype, lead=5, trail=7, junk=jk, kernel=kernel, what="lead 5 trail 7")
    check_all(p, o, rows, dtype, lead=0, trail=0, junk=jk, what="offsets[0] = 0, last row at the tensor's end")
    check_all(p, o, rows, dtype, lead=133, trail=0, junk=jk, what="offsets[0] > 0, last row at the tensor's end")
    for n in (1, 63, 65, 130):                      # batches ending inside a 64-row group
        check_all(p, o, rows[48:48 + n], dtype, lead=3, trail=5, junk=jk, what="n_rows %d" % n)
    check_all(p, o, [np.zeros(0, dtype)] * 70, dtype, lead=9, trail=9, junk=jk, what="only empty rows")


def decode_form(ft):
    """Which of the lock-step decode's five forms (needle_find_all_ls_walk.h find_all_ls_decode) a transducer program takes, read off its
    codes table as the lowering numbers it (needle_lower.cpp): codes[c] = (k + length) | k << 16, codes[0] = 0."""
    if ft["kind"] == 2:
        return "run", 0
    codes = ft["blob"][ft["codes_off"]:ft["codes_off"] + 64].view(np.uint32)
    assert codes[0] == 0
    used = [(c, int(d >> 16), int(d & 0xFFFF) - int(d >> 16)) for c, d in enumerate(codes) if d]  # (code, k, length)
    if all(k == 0 and 1 <= length <= 7 for _, k, length in used):
        assert all(c == 2 * length + 1 for c, _, length in used)
        return "direct 2", len(used)
    if all(k == 0 and 1 <= length <= 15 for _, k, length in used):
        assert all(c == length for c, _, length in used)
        return "direct 1", len(used)
    assert any(k > 0 for _, k, _ in used)          # (what keeps these patterns off the direct forms)
    if len(used) <= 8:
        assert all(c % 2 == 1 for c, _, _ in used)
        return "table, odd codes", len(used)
    return "table", len(used)


DECODE_FORMS = [
    # (regex, char widths, form, codes, a match, adjacent matches: several ends within 8 chars)
    ("[0-9]+", (1, 2), "run", 0, "0123", "1 22 3 4 55 6 7 "),
    ("[α-ω]{2}[α-ω]*", (2,), "run", 0, "αβγ", "αβ γω αβ ωω αβγ "),
    ("Sherlock|Holmes|Watson|Irene|Adler|John|Baker", (1, 2), "direct 1", None, "Sherlock", "JohnJohnJohnIrene"),
    ("a.c|ab", (1, 2), "direct 2", None, "axc", "ababababab"),
    ("abcdefgh|abcd", (1, 2), "table, odd codes", 5, "abcdefgh", "abcdabcdabcdabcd"),
    ("abcdefghijklmno|abc|abcdefg|abcdefghijk", (1, 2), "table", 13, "abcdefghijklmno", "abcabcabcabcabc"),
]


@pytest.mark.gpu
@pytest.mark.parametrize("regex,cw,form,n_codes,word,dense", [(rx, cw, f, nc, w, d) for rx, cws, f, nc, w, d in DECODE_FORMS for cw in cws])
def test_every_decode_form_in_both_layouts(regex, cw, form, n_codes, word, dense):
    """The five forms of the lock-step decode, each on packed rows and (check_all) on the same rows at a fixed stride: a lowering change
    that moves a pattern to another form fails here instead of dropping the form's coverage."""
    p, o = compiled(regex)
    dtype = np.uint8 if cw == 1 else np.uint16
    got_form, got_codes = decode_form(p.find_all_transducer(cw))
    assert got_form == form and (n_codes is None or got_codes == n_codes), (got_form, got_codes)
    rng = np.random.default_rng(len(regex) + cw)
    arr = lambda s: np.array([ord(ch) for ch in s], dtype)
    letters = arr("".join(sorted(set(ch for ch in regex + word + dense if ch.isalnum()))) + " ")
    pieces = [arr(word), arr(word[:-1]), arr(dense), arr(" ")]
    def row(n):
        parts, have = [], 0
        while have < n:
            parts.append(pieces[int(rng.integers(0, 4))] if rng.random() < 0.6 else rng.choice(letters, int(rng.integers(1, 9))))
            have += parts[-1].size
        return np.concatenate(parts)[:n].astype(dtype) if parts else np.zeros(0, dtype)
    rows = [row(int(n)) for n in rng.integers(0, 301, 130)]
    rows[0] = np.zeros(0, dtype)
    rows[1] = arr("  " + word)                               # ends with a match's last char: emitted by the PAD transition
    rows[2] = arr("  " + word[:-1])                          # cut one char short
    rows[3] = arr(dense * 3)
    rows[129] = row(300)
    per16 = 16 // cw                                         # 16 rows of 33 chars: their ends take every position in a 16-byte block,
    for i in range(64, 80):                                  # so one ends on a block boundary of the buffer whatever the lead is
        rows[i] = arr(" " * (33 - len(word)) + word)
    ends = np.cumsum([len(r) for r in rows])[64:80]
    assert len(set((ends % per16).tolist())) == per16
    for lead in (5, 0):             # (check_all compares every GPU result with the oracle; it returns the ORACLE's matches)
        off, st, en = check_all(p, o, rows, dtype, lead=lead, trail=7, junk=arr(word).tolist(), kernel=True, what="lead %d" % lead)
    # not result checks: the input holds what it was built to hold, by the oracle's matches (the same for either lead)
    assert off[2] - off[1] >= 1 and en[off[2] - 1] == len(rows[1])      # a match that ends with its row
    assert off[4] - off[3] >= 6                                         # adjacent matches
    assert (np.diff(off)[64:80] >= 1).all() and (en[off[65:81] - 1] == 33).all()


@pytest.mark.gpu
def test_c5_script_runs_utf16():
    from needle_amd import workload as W
    import torch
    p, o = compiled(W.script_regex())
    assert p.find_all_transducer(2) is not None
    rows = W.script_batch(torch, 0, 600, 200).cpu().numpy().astype(np.uint16)
    lens = np.random.default_rng(3).integers(0, 201, 600)
    check_all(p, o, [rows[i, :lens[i]] for i in range(600)], np.uint16, lead=6, trail=2, junk=[0x5900, 0x5901, 0x5902], kernel=True)


@pytest.mark.gpu
@pytest.mark.parametrize("regex,cw", [("[0-9]+", 1), ("Sherlock|Holmes", 1), ("[α-ω]{2}[α-ω]*", 2), ("a.c", 2)])
def test_windows_and_row_ends(regex, cw):
    """Rows spanning several windows, matches straddling window edges (runs across every 64-byte / 128-byte lane boundary),
    matches pending at the row's end, rows starting and ending mid-block, and one row over 1 MiB among short rows."""
    p, o = compiled(regex)
    dtype = np.uint8 if cw == 1 else np.uint16
    word = {"[0-9]+": "0123456789", "Sherlock|Holmes": "Holmes", "[α-ω]{2}[α-ω]*": "αβγδε", "a.c": "abc"}[regex]
    w = np.array([ord(c) for c in word], dtype)
    sep = np.array([ord(" ")], dtype)
    rng = np.random.default_rng(5)
    rows = []
    for i in range(200):
        k = int(rng.integers(0, 900))                       # up to ~9 KiB: several 4 / 8 KiB windows
        parts = []
        while sum(x.size for x in parts) < k:
            parts.append(np.resize(w, int(rng.integers(1, 3 * w.size + 1))))
            if rng.random() < 0.5:
                parts.append(sep)
        r = np.concatenate(parts)[:k] if parts else np.zeros(0, dtype)
        rows.append(r.astype(dtype))
    rows[17] = np.resize(w, 6000).astype(dtype)             # one match (or run) across every window edge of its span
    rows[18] = np.concatenate([np.full(3, ord(" "), dtype), np.resize(w, 5000 + w.size - 1)]).astype(dtype)  # pending at the end
    check_all(p, o, rows, dtype, lead=7, trail=3, junk=w.tolist())
    big = np.resize(np.concatenate([w, sep, w[:1], sep]), (1 << 20) + 37).astype(dtype)
    rows2 = rows[:40] + [big] + rows[40:90]
    check_all(p, o, rows2, dtype, lead=1, trail=0, junk=w.tolist(), what="one row > 1 MiB")
    if p.find_all_transducer(cw) is not None:                # the one-dword form refuses rows over 65 535 chars (asked with `more`)
        from needle_amd.pattern import PatternException, DeviceError
        data, offsets = device_packed(rows2, dtype)
        with pytest.raises((PatternException, DeviceError, RuntimeError, ValueError)):
            p.find_all_compact16_packed(data, offsets)


@pytest.mark.gpu
def test_compact16_refused_without_transducer_and_host_capacity_retry():
    import torch
    p, o = compiled("international|inter|nation")
    data, offsets = device_packed([np.frombuffer(b"international", np.uint8)] * 3, np.uint8)
    with pytest.raises(Exception, match="needle_find_all_csr_packed_dev"):
        p.find_all_compact16_packed(data, offsets)
    # the host entry's capacity retry: far more matches than its first guess (2 per row)
    q, qo = compiled("[0-9]")
    rows = [np.full(50, ord("7"), np.uint8) for _ in range(300)] + [np.zeros(0, np.uint8)]
    offs = np.zeros(len(rows) + 1, np.uint64)
    offs[1:] = np.cumsum([r.size for r in rows])
    ho, hs, he = q.find_all_packed(np.concatenate(rows), offs)
    want = flatten(oracle_all(qo, rows))
    assert ho[-1] == 15000 and (ho == want[0]).all() and (hs == want[1]).all() and (he == want[2]).all()
    # Python str lists (UTF-16, like java.lang.String[])
    r, ro = compiled("[α-ω]+|ab")
    strs = ["", "abαβ xab", "ωω", "no", "ab" * 40, "αab"]
    got = r.find_all_strings(strs)
    assert got == [ro.find_all(np.array([ord(c) for c in s], np.uint16), limit=1 << 30) for s in strs]
    assert got[1] == [(0, 2), (2, 4), (6, 8)]


@pytest.mark.gpu
def test_non_default_stream():
    """Everything on a fresh stream, the results read right after the calls with no extra synchronisation of the device."""
    import torch
    p, o = compiled("[0-9]+")
    rng = np.random.default_rng(2)
    rows = layout_rows(rng, [ord(c) for c in "ab 0123456789"], [], n=3000, max_len=300)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        check_all(p, o, rows, np.uint8, stream=s.cuda_stream, what="stream")


@pytest.mark.gpu
def test_ten_million_ragged_rows():
    """c2p / c3p: the bench generators' 10^7 rows, lengths (r * 2654435761) % 256 + 1, packed.  Total count and checksum equal the
    fixed-stride ragged route on the same rows; compact16 equals too; the oracle checks sampled rows."""
    import torch
    from needle_amd import workload as W
    n = 10_000_000
    dev = torch.device("cuda")
    lens = (torch.arange(n, device=dev, dtype=torch.int64) * 2654435761 % 256 + 1)
    offsets = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    offsets[1:] = torch.cumsum(lens, 0)
    col = torch.arange(256, device=dev)[None, :]
    sample = np.random.default_rng(1).choice(n, 1500, replace=False)
    words = W.keywords(1000)
    for name, rx, gen in (("c2p", "[0-9]+", lambda r0, k: W.digits_batch(torch, r0, k, 256, device=dev)),
                          ("c3p", "|".join(words), lambda r0, k: W.keyword_batch(torch, words, r0, k, 256, device=dev))):
        p, o = compiled(rx)
        assert p.find_all_transducer(1) is not None, name
        rows = torch.empty((n, 256), dtype=torch.uint8, device=dev)
        for s in range(0, n, 1 << 19):
            k = min(1 << 19, n - s)
            rows[s:s + k] = gen(s, k)
        data = torch.empty(int(offsets[-1].item()), dtype=torch.uint8, device=dev)
        for s in range(0, n, 1 << 20):
            k = min(1 << 20, n - s)
            data[int(offsets[s].item()):int(offsets[s + k].item())] = rows[s:s + k][col < lens[s:s + k, None]]
        l32 = lens.to(torch.int32)
        go, gs, ge = p.find_all_packed(data, offsets)
        wo, ws, we = p.find_all_csr(rows, l32)
        torch.cuda.synchronize()
        assert int(go[-1]) == int(wo[-1]) and int(go[-1]) > 0, name
        csum = lambda s, e: int((s.to(torch.int64) * 1000003 + e.to(torch.int64)).sum())
        assert csum(gs, ge) == csum(ws, we), name
        assert torch.equal(go, wo) and torch.equal(gs, ws) and torch.equal(ge, we), name
        co, cse, cm = p.find_all_compact16_packed(data, offsets, max_per_row=64)
        fo, fse, fm = p.find_all_compact16(rows, max_per_row=64, lengths=l32)
        torch.cuda.synchronize()
        assert torch.equal(co, fo) and torch.equal(cse, fse) and cm == fm, name
        goc, wsn = go.cpu().numpy(), None
        gsc, gec = gs.cpu().numpy(), ge.cpu().numpy()
        srows = rows[torch.from_numpy(sample).to(dev)].cpu().numpy()
        slens = lens.cpu().numpy()[sample]
        for j, r in enumerate(sample):
            want = o.find_all(srows[j, :slens[j]], limit=1 << 30)
            got = list(zip(gsc[goc[r]:goc[r + 1]].tolist(), gec[goc[r]:goc[r + 1]].tolist()))
            assert got == want, (name, r)
        del rows, data


ALPHABET = [ord(c) for c in "abcxyz019 AB_\n."] + [0xE9, 0x416, 0x4E2D, 0xFFFF]


@pytest.mark.gpu
@pytest.mark.parametrize("seed", range(20))
def test_fuzz_regexes_and_dictionaries(seed):
    """Seeded random regexes (drawn as tests/test_gpu_fuzz.py draws them) and random dictionaries over random packed batches and
    offsets, 8- and 16-bit: 2 regexes + 1 dictionary per seed."""
    from needle_amd.pattern import PatternException
    from test_compile_vs_python_restatement import FLAG_SETS, random_regex
    rng = random.Random(7300 + seed)
    nrng = np.random.default_rng(seed)
    done = 0
    while done < 2:
        regex, flags = random_regex(rng), rng.choice(FLAG_SETS)
        try:
            p, o = compiled(regex, flags)
        except (PatternException, ValueError):
            continue
        done += 1
        rows16 = layout_rows(nrng, ALPHABET, [], n=300, max_len=90, dtype=np.uint16)
        check_all(p, o, rows16, np.uint16, lead=int(nrng.integers(0, 9)), trail=int(nrng.integers(0, 2)) * 5, junk=ALPHABET, what=(regex, flags))
        rows8 = layout_rows(nrng, [c for c in ALPHABET if c < 256], [], n=300, max_len=150)
        check_all(p, o, rows8, np.uint8, lead=int(nrng.integers(0, 9)), trail=3, junk=[c for c in ALPHABET if c < 256], what=(regex, flags))
    letters = "abcdefgh"
    words = sorted({"".join(rng.choice(letters) for _ in range(rng.randint(2, 7))) for _ in range(rng.randint(5, 60))})
    rng.shuffle(words)
    p, o = compiled("|".join(words))
    rows = layout_rows(nrng, [ord(ch) for ch in letters + " "], words, n=1200, max_len=200)
    check_all(p, o, rows, np.uint8, lead=int(nrng.integers(0, 40)), trail=3, junk=[ord(ch) for ch in words[0]], what=("dictionary", words[:5]))
