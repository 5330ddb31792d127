"""Packed device batches scanned as they lie (needle_matches_packed_dev / needle_contained_in_packed_dev / needle_find_packed_dev,
the kernel of needle_packed.h): every case against the oracle walking the same tables on each row, and against
rows_from_packed followed by the fixed-stride entries on the same rows -- bit for bit, start / end for every row.

Layouts: empty rows and runs of them, every row length and start offset mod 16, partial last groups, offsets[0] > 0 with
pattern-matching text before offsets[0] and after offsets[n] in the same tensor (an over-read changes answers), the last row
ending at the 4-byte-padded end of the tensor, long rows among short ones, a non-default stream, 10^7 ragged rows."""
import os
import random
import subprocess
import sys

import numpy as np
import pytest

from test_gpu_configs import compiled

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------------------------------------------------------------------
# helpers
def oracle_packed(o, rows, dtype):
    """(matches, containedIn, found, start, end) of every row by the oracle; rows bucketed by length so that the padded copies
    stay small whatever the mix."""
    n = len(rows)
    lens = np.array([len(r) for r in rows], dtype=np.int64)
    m, c, f = np.zeros(n, bool), np.zeros(n, bool), np.zeros(n, bool)
    s, e = np.full(n, -1, np.int32), np.full(n, -1, np.int32)
    klass = np.zeros(n, np.int64)
    for k in range(1, 16):
        klass[lens > (64 << (2 * (k - 1)))] = k
    for k in np.unique(klass):
        idx = np.nonzero(klass == k)[0]
        width = max(1, int(lens[idx].max()))
        pad = np.zeros((idx.size, width), dtype=dtype)
        for j, i in enumerate(idx):
            pad[j, :lens[i]] = rows[i]
        L = lens[idx].astype(np.uint32)
        m[idx] = o.batch_matches(pad, L, threads=8)
        c[idx] = o.batch_contained_in(pad, L, threads=8)
        f[idx], s[idx], e[idx] = o.batch_find(pad, L, threads=8)
    return m, c, f, s, e


def device_packed(rows, dtype, lead=5, trail=7, junk=None):
    """Device (data, offsets): `lead` junk code units before offsets[0] (rounded up so that the text ends on a 4-byte boundary
    when trail == 0: the last row then ends exactly at the tensor's end), the rows back to back, `trail` junk units after."""
    import torch
    cw = np.dtype(dtype).itemsize
    lens = np.array([len(r) for r in rows], dtype=np.int64)
    total = int(lens.sum())
    per4 = 4 // cw
    lead = lead + (-(lead + total + trail)) % per4
    junk = np.zeros(1, dtype) if junk is None else np.asarray(junk, dtype=dtype)
    fill = lambda k: np.resize(junk, k).astype(dtype)
    parts = [fill(lead)] + [np.asarray(r, dtype=dtype) for r in rows] + [fill(trail)]
    host = np.concatenate(parts) if parts else np.zeros(0, dtype)
    assert (host.size * cw) % 4 == 0
    offsets = np.zeros(len(rows) + 1, dtype=np.int64)
    offsets[1:] = np.cumsum(lens)
    offsets += lead
    tdt = torch.uint8 if cw == 1 else torch.int16
    data = torch.from_numpy(host.view(np.uint8) if cw == 1 else host.view(np.int16)).to("cuda")
    assert data.dtype == tdt
    return data, torch.from_numpy(offsets).to("cuda")


def run_packed(p, data, offsets, stream=None):
    import torch
    m = p.matches_packed(data, offsets, stream=stream)
    c = p.contained_in_packed(data, offsets, stream=stream)
    f = p.find_packed(data, offsets, stream=stream)
    if stream is None:
        torch.cuda.synchronize()
    assert isinstance(m, torch.Tensor) and m.is_cuda and isinstance(f[1], torch.Tensor) and f[1].is_cuda
    return m, c, f


def check(p, o, rows, dtype, lead=5, trail=7, junk=None, fixed=True, what=""):
    from needle_amd.pattern import Pattern, unpack_bitmap
    n = len(rows)
    data, offsets = device_packed(rows, dtype, lead, trail, junk)
    m, c, (fw, fs, fe) = run_packed(p, data, offsets)
    gm, gc, gf = unpack_bitmap(m, n), unpack_bitmap(c, n), unpack_bitmap(fw, n)
    gs, ge = fs.cpu().numpy(), fe.cpu().numpy()
    wm, wc, wf, ws, we = oracle_packed(o, rows, dtype)
    for name, got, want in (("matches", gm, wm), ("containedIn", gc, wc), ("find", gf, wf), ("start", gs, ws), ("end", ge, we)):
        bad = np.nonzero(got != want)[0]
        assert bad.size == 0, (what, name, bad[:10], [len(rows[i]) for i in bad[:10]], got[bad[:5]], want[bad[:5]])
    # the fixed-stride entries on the same rows (what a packed device batch cost before): the same bits, word for word
    longest = max([len(r) for r in rows] + [1])
    if fixed and n * longest * np.dtype(dtype).itemsize <= (1 << 29):
        rt, lt, ovf = Pattern.rows_from_packed(data, offsets)
        xm = p.matches_batch(rt, lt)
        xc = p.contained_in_batch(rt, lt)
        xf, xs, xe = p.find_batch(rt, lt)
        nw = (n + 63) // 64
        assert int(ovf.item()) == 0
        assert (m[:nw].cpu().numpy() == xm[:nw].cpu().numpy()).all(), what
        assert (c[:nw].cpu().numpy() == xc[:nw].cpu().numpy()).all(), what
        assert (fw[:nw].cpu().numpy() == xf[:nw].cpu().numpy()).all(), what
        assert (fs.cpu().numpy() == xs.cpu().numpy()).all() and (fe.cpu().numpy() == xe.cpu().numpy()).all(), what
    return gm, gc, gf


def layout_rows(rng, alphabet, plants, n=1000, max_len=120, dtype=np.uint8):
    """Rows of every length mod 16 (so every start offset mod 16 follows), runs of empty rows, planted words anywhere."""
    lens = rng.integers(0, max_len + 1, n)
    lens[:48] = np.arange(48)                      # every small length, hence every start mod 16
    lens[100:110] = 0                              # a run of empty rows
    lens[200:264] = 0                              # a whole group of empty rows
    rows = []
    alphabet = np.asarray(alphabet)
    for i, l in enumerate(lens):
        r = rng.choice(alphabet, int(l)).astype(dtype)
        if plants and l and rng.random() < 0.4:
            w = np.array([ord(ch) for ch in rng.choice(plants)], dtype=dtype)
            at = int(rng.integers(0, max(1, l - w.size + 1)))
            k = min(w.size, l - at)
            r[at:at + k] = w[:k]
        rows.append(r)
    return rows


PATTERNS = [
    # (regex, char width, alphabet, planted words, junk that matches)
    ("[0-9]+", 1, "abcxyz 0123456789", [], "0123"),
    ("Sherlock|Holmes|Watson|Irene|Adler|John|Baker", 1, "SherlockHmsWatnIdJB ", ["Sherlock", "Holmes", "Baker"], "Holmes"),
    ("http://.+", 1, "htp:/abc.x\n", ["http://", "http://a.b"], "http://x"),
    ("a.c", 1, "abcx\n", ["abc", "axc"], "abc"),
    ("[a-c]*", 1, "abcd", [], "abc"),
    ("[α-ω]{2}[α-ω]*", 2, "ab αβω￿", ["αβγ"], "αβγ"),
    ("[a-z一-丠]+[0-9]|ЖЗ+", 2, "az9一丐丰ЖЗ ", ["一丁x7", "ЖЗЗ"], "一a1"),
]


def _compiled_dictionary(n_words=300):
    from needle_amd import workload as W
    words = W.keywords(n_words)
    p, o = compiled("|".join(words))
    return p, o, words


# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("regex,cw,alphabet,plants,junk", PATTERNS)
def test_patterns_and_layouts(regex, cw, alphabet, plants, junk):
    p, o = compiled(regex)
    dtype = np.uint8 if cw == 1 else np.uint16
    rng = np.random.default_rng(7 + len(regex))
    al = [ord(ch) for ch in alphabet]
    jk = [ord(ch) for ch in junk]
    rows = layout_rows(rng, al, plants, dtype=dtype)
    check(p, o, rows, dtype, lead=5, trail=7, junk=jk, what="lead 5 trail 7")
    check(p, o, rows, dtype, lead=0, trail=0, junk=jk, what="offsets[0] = 0, last row at the tensor's end")
    check(p, o, rows, dtype, lead=133, trail=0, junk=jk, what="offsets[0] > 0, last row at the tensor's end")
    for n in (1, 63, 64, 65, 130, 200):            # partial and whole groups
        check(p, o, rows[48:48 + n], dtype, lead=3, trail=5, junk=jk, what="n_rows %d" % n)
    check(p, o, [np.zeros(0, dtype)] * 70, dtype, lead=9, trail=9, junk=jk, what="only empty rows")


@pytest.mark.gpu
def test_dictionary_300_keywords_lengths_form():
    from needle_amd import workload as W
    p, o, words = _compiled_dictionary(300)
    assert p.info()["kernel_mode"]["forwards"] in (1, 2, 4, 6)  # an LDS program: the lengths form serves find()
    rng = np.random.default_rng(3)
    rows = layout_rows(rng, [ord(ch) for ch in "abcdefghijklmnopqrstuvwxyz "], words, n=3000, max_len=200)
    check(p, o, rows, np.uint8, lead=11, trail=11, junk=[ord(ch) for ch in words[0]])
    rows16 = [r.astype(np.uint16) for r in rows]
    check(p, o, rows16, np.uint16, lead=6, trail=0, junk=[ord(ch) for ch in words[1]])


# every device program the tiled scan runs, forced in child processes by the switches the existing tests use
# (env, kernel_mode of the 300-keyword dictionary, of the 7-keyword union -- None: not asserted)
FORCED = [
    ({"NEEDLE_MAX_PROG_LDS": "4096", "NEEDLE_HYBRID": "0", "NEEDLE_SPARSE": "0"}, 3, None),   # HBM table
    ({"NEEDLE_MAX_PROG_LDS": "4096", "NEEDLE_SPARSE": "0"}, 5, None),                          # hot rows + HBM table
    ({"NEEDLE_MAX_PROG_LDS": "20000", "NEEDLE_SPARSE": "1"}, 6, None),                         # compressed automaton
    ({"NEEDLE_MAX_PROG_LDS": "20000", "NEEDLE_SPARSE": "0"}, 5, None),                         # hot rows
    ({"NEEDLE_PAIR_MAX_BYTES": "0"}, None, 1),                                                 # the union as a u8 table, not pairs
    ({"NEEDLE_FIND_LENGTHS": "0"}, 2, 4),                                                      # find() by backward walks
]
CHILD = r'''
import sys
sys.path.insert(0, "."); sys.path.insert(0, "tests")
import numpy as np
import test_gpu_packed_dev as T
p, o, words = T._compiled_dictionary(300)
want, want7 = int(sys.argv[1]), int(sys.argv[2])
mode = p.info()["kernel_mode"]["forwards"]
assert want < 0 or mode == want, (mode, want)
mode7 = T.compiled("Sherlock|Holmes|Watson|Irene|Adler|John|Baker")[0].info()["kernel_mode"]["forwards"]
assert want7 < 0 or mode7 == want7, (mode7, want7)
rng = np.random.default_rng(5)
rows = T.layout_rows(rng, [ord(ch) for ch in "abcdefghijklmnopqrstuvwxyz "], words, n=1500, max_len=300)
T.check(p, o, rows, np.uint8, lead=7, trail=3, junk=[ord(ch) for ch in words[0]])
T.check(p, o, [r.astype(np.uint16) for r in rows[:700]], np.uint16, lead=2, trail=0, junk=[ord(ch) for ch in words[2]])
for rx in ("Sherlock|Holmes|Watson|Irene|Adler|John|Baker", "http://.+"):
    p2, o2 = T.compiled(rx)
    rows2 = T.layout_rows(rng, [ord(ch) for ch in "SherlockHmsWatnIdJBhtp:/."], ["Sherlock", "Holmes", "http://a"], n=700)
    T.check(p2, o2, rows2, np.uint8, lead=4, trail=4, junk=[ord(ch) for ch in "Holmes"])
print("PACKED-DEV-CHILD-OK mode", mode)
'''


@pytest.mark.gpu
@pytest.mark.parametrize("env,mode,mode7", FORCED)
def test_forced_device_programs(env, mode, mode7):
    r = subprocess.run([sys.executable, "-c", CHILD, str(-1 if mode is None else mode), str(-1 if mode7 is None else mode7)], env=dict(os.environ, **env),
                       capture_output=True, text=True, timeout=900, cwd=ROOT)
    assert "PACKED-DEV-CHILD-OK" in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]


@pytest.mark.gpu
def test_long_rows():
    """5 KiB, 100 KiB and 1 MiB rows among 10 000 short ones and on their own: spans far wider than a wave's window; digit runs at
    row starts, at row ends, across every 4 KiB / 8 KiB boundary of the row, and nowhere."""
    p, o = compiled("[0-9]+")
    rng = np.random.default_rng(17)
    letters = np.array([ord(ch) for ch in "abcdefxyz "], dtype=np.uint8)

    def long_row(n, where):
        r = rng.choice(letters, n).astype(np.uint8)
        if where == "start":
            r[:3] = ord("7")
        elif where == "end":
            r[-2:] = ord("5")
        elif where == "edges":
            for k in range(4096 - 3, n - 3, 4096):
                r[k:k + 5] = ord("1")
        return r
    longs = [long_row(n, w) for n in (5 << 10, 100 << 10, 1 << 20) for w in ("start", "end", "edges", "none")]
    short = layout_rows(rng, [ord(ch) for ch in "abcxyz 019"], [], n=10000, max_len=60)
    rows = list(short)
    for k, r in enumerate(longs):
        rows.insert(37 + k * 811, r)
    check(p, o, rows, np.uint8, lead=13, trail=9, junk=[ord("9")], fixed=False, what="long among short")
    check(p, o, longs, np.uint8, lead=1, trail=0, junk=[ord("9")], what="long rows only")
    check(p, o, [r.astype(np.uint16) for r in longs[:8]], np.uint16, lead=1, trail=3, junk=[ord("9")], what="long rows, 16-bit")


@pytest.mark.gpu
def test_early_exit_batches():
    """Nearly every row matching in its first chars (groups resolve at once) and rows matching only at their last char."""
    p, o = compiled("[0-9]+")
    rng = np.random.default_rng(23)
    letters = [ord(ch) for ch in "abcdefxyz "]
    first = [np.concatenate([[ord("4")], rng.choice(letters, int(l))]).astype(np.uint8) for l in rng.integers(0, 3000, 3000)]
    first[::97] = [rng.choice(letters, 500).astype(np.uint8) for _ in first[::97]]
    check(p, o, first, np.uint8, lead=2, trail=2, junk=[ord("1")], what="match at the first char")
    last = [np.concatenate([rng.choice(letters, int(l)), [ord("8")]]).astype(np.uint8) for l in rng.integers(0, 3000, 3000)]
    check(p, o, last, np.uint8, lead=2, trail=2, junk=[ord("1")], what="match at the last char")
    pk, ok, words = _compiled_dictionary(300)
    kw = [np.array([ord(ch) for ch in words[i % 300] + "zz" * int(rng.integers(0, 400))], dtype=np.uint8) for i in range(3000)]
    check(pk, ok, kw, np.uint8, lead=2, trail=2, junk=[ord(ch) for ch in words[0]], what="keyword at the start")


@pytest.mark.gpu
def test_non_default_stream():
    import torch
    from needle_amd.pattern import unpack_bitmap
    p, o = compiled("[0-9]+")
    rng = np.random.default_rng(31)
    rows = layout_rows(rng, [ord(ch) for ch in "abc 0123"], [], n=5000, max_len=300)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        data, offsets = device_packed(rows, np.uint8, 3, 3, [ord("5")])
        c = p.contained_in_packed(data, offsets, stream=s.cuda_stream)
        fw, fs, fe = p.find_packed(data, offsets, stream=s.cuda_stream)
    s.synchronize()
    _, wc, wf, ws, we = oracle_packed(o, rows, np.uint8)
    assert (unpack_bitmap(c, len(rows)) == wc).all() and (unpack_bitmap(fw, len(rows)) == wf).all()
    assert (fs.cpu().numpy() == ws).all() and (fe.cpu().numpy() == we).all()
    # out=: caller-owned buffers
    n = len(rows)
    bm = torch.full(((n + 63) // 64,), -1, dtype=torch.int64, device="cuda")
    st = torch.empty(n, dtype=torch.int32, device="cuda")
    en = torch.empty(n, dtype=torch.int32, device="cuda")
    r = p.find_packed(data, offsets, out=(bm, st, en))
    torch.cuda.synchronize()
    assert r[0] is bm and (unpack_bitmap(bm, n) == wf).all() and (st.cpu().numpy() == ws).all()


@pytest.mark.gpu
def test_ten_million_ragged_rows():
    """bench.py's ragged batch (c2r / c3r: the same generators, lengths (r * 2654435761) % 256 + 1), packed: the packed calls equal
    the fixed-stride ragged calls on the same rows, plus the oracle on a sample."""
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
    words = W.keywords(1000)
    for name, rx, gen in (("c2p", "[0-9]+", lambda r0, k: W.digits_batch(torch, r0, k, 256, device=dev)),
                          ("c3p", "|".join(words), lambda r0, k: W.keyword_batch(torch, words, r0, k, 256, device=dev))):
        p, o = compiled(rx)
        rows = torch.empty((n, 256), dtype=torch.uint8, device=dev)
        for s in range(0, n, 1 << 19):
            k = min(1 << 19, n - s)
            rows[s:s + k] = gen(s, k)
        data = torch.empty(int(offsets[-1].item()), dtype=torch.uint8, device=dev)
        for s in range(0, n, 1 << 20):  # (packed slab by slab: a boolean mask over all 2.56 G chars is beyond torch's indexing)
            k = min(1 << 20, n - s)
            data[int(offsets[s].item()):int(offsets[s + k].item())] = rows[s:s + k][col < lens[s:s + k, None]]
        l32 = lens.to(torch.int32)
        if name == "c2p":
            got = p.contained_in_packed(data, offsets)
            want = p.contained_in_batch(rows, l32)
            torch.cuda.synchronize()
            assert torch.equal(got, want), name
        else:
            gw, gs, ge = p.find_packed(data, offsets)
            ww, ws, we = p.find_batch(rows, l32)
            torch.cuda.synchronize()
            assert torch.equal(gw, ww) and torch.equal(gs, ws) and torch.equal(ge, we), name
        # the oracle on sampled rows
        srows = rows[sample].cpu().numpy()
        slens = lens[sample].cpu().numpy().astype(np.uint32)
        idx = sample.cpu().numpy()
        if name == "c2p":
            assert (unpack_bitmap(got, n)[idx] == o.batch_contained_in(srows, slens, threads=8)).all()
        else:
            of, os_, oe = o.batch_find(srows, slens, threads=8)
            assert (unpack_bitmap(gw, n)[idx] == of).all()
            assert (gs[sample].cpu().numpy() == os_).all() and (ge[sample].cpu().numpy() == oe).all()
        del rows, data


ALPHABET = [ord(c) for c in "abcxyz019 AB_\n."] + [0xE9, 0x416, 0x4E2D, 0xFFFF]


@pytest.mark.gpu
@pytest.mark.parametrize("seed", range(6))
def test_fuzz_regexes_and_dictionaries(seed):
    """Seeded random regexes (drawn as tests/test_gpu_fuzz.py draws them) and random dictionaries over random packed batches,
    8- and 16-bit: 4 regexes + 1 dictionary per seed."""
    from needle_amd.pattern import PatternException
    from test_compile_vs_python_restatement import FLAG_SETS, random_regex
    rng = random.Random(9000 + seed)
    nrng = np.random.default_rng(seed)
    done = 0
    while done < 4:
        regex, flags = random_regex(rng), rng.choice(FLAG_SETS)
        try:
            p, o = compiled(regex, flags)
        except (PatternException, ValueError):
            continue
        done += 1
        rows16 = layout_rows(nrng, ALPHABET, [], n=400, max_len=90, dtype=np.uint16)
        check(p, o, rows16, np.uint16, lead=int(nrng.integers(0, 9)), trail=int(nrng.integers(0, 2)) * 5, junk=ALPHABET, what=(regex, flags))
        rows8 = layout_rows(nrng, [c for c in ALPHABET if c < 256], [], n=400, max_len=150)
        check(p, o, rows8, np.uint8, lead=int(nrng.integers(0, 9)), trail=3, junk=[c for c in ALPHABET if c < 256], what=(regex, flags))
    letters = "abcdefgh"
    words = sorted({"".join(rng.choice(letters) for _ in range(rng.randint(2, 7))) for _ in range(rng.randint(5, 60))})
    rng.shuffle(words)
    p, o = compiled("|".join(words))
    rows = layout_rows(nrng, [ord(ch) for ch in letters + " "], words, n=1500, max_len=200)
    check(p, o, rows, np.uint8, lead=3, trail=3, junk=[ord(ch) for ch in words[0]], what=("dictionary", words[:5]))
