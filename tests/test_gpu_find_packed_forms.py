"""The rest of find()'s surface for packed device batches (needle_find_next_packed_dev, needle_find_packed{16,8}_packed_dev and
_host): the compact forms against needle_find_packed_dev packed row by row (escapes exactly on rows whose match ends past 65 534 /
256, the overflow flag exactly when some row escaped), the cursor entry against the oracle's find(h, start=c) and against
find_next_batch on rows_from_packed output, the enumeration by feeding `end` back, the host entries against the device ones,
streams and caller-owned outputs, and 10^7 ragged rows.

Patterns: every program the int32 packed entry meets -- fixed length, a lengths-form dictionary, backward walks, nullable /
root-accepting, packed functions, the pair table, the compressed automaton of a C3-sparse-sized dictionary, the C5 class regex.
Layouts: 8- and 16-bit rows, empty rows, every start offset mod 16, partial last groups, offsets[0] > 0 with matching junk around
the rows, the last row ending at the tensor's end."""
import numpy as np
import pytest

from test_gpu_configs import compiled
from test_gpu_packed_dev import device_packed, layout_rows

PACK16_OVER, PACK8_OVER = 0xFFFEFFFF, 0xFFFD


# ---------------------------------------------------------------------------------------------------------------------------
# helpers
def pack16_expected(st, en):
    st, en = st.astype(np.int64), en.astype(np.int64)
    return np.where(en < 0, 0xFFFFFFFF, np.where(en <= 65534, (st & 0xFFFF) | (en << 16), PACK16_OVER)).astype(np.uint32)


def pack8_expected(st, en):
    """needle_device.h pack8() where end <= 256, the escape beyond."""
    st, en = st.astype(np.int64), en.astype(np.int64)
    ln = (en - st) & 0xFFFFFFFF
    held = np.where(ln > 255, 0xFFFE, (st & 0xFF) | (ln << 8))
    return np.where(en < 0, 0xFFFF, np.where(en <= 256, held, PACK8_OVER)).astype(np.uint16)


def check_forms(p, rows, dtype, lead=5, trail=7, junk=None, host=True, what=""):
    """The 16- and 8-bit forms (device, and host where every row fits) against the int32 entry on the same packed rows."""
    import torch
    n = len(rows)
    data, offsets = device_packed(rows, dtype, lead, trail, junk)
    w, s, e = p.find_packed(data, offsets)
    w16, r16, o16 = p.find_packed16_packed(data, offsets)
    w8, r8, o8 = p.find_packed8_packed(data, offsets)
    torch.cuda.synchronize()
    nw = (n + 63) // 64
    s, e = s.cpu().numpy(), e.cpu().numpy()
    assert torch.equal(w16[:nw], w[:nw]) and torch.equal(w8[:nw], w[:nw]), ("bitmap", what)
    g16 = r16.cpu().numpy().view(np.uint32)
    g8 = r8.cpu().numpy().view(np.uint16)
    for name, got, want in (("16", g16, pack16_expected(s, e)), ("8", g8, pack8_expected(s, e))):
        bad = np.nonzero(got != want)[0]
        assert bad.size == 0, (what, name, bad[:8], got[bad[:4]], want[bad[:4]], s[bad[:4]], e[bad[:4]])
    assert int(o16.item()) == int((e > 65534).any()), ("overflow16", what)
    assert int(o8.item()) == int((e > 256).any()), ("overflow8", what)
    longest = max([len(r) for r in rows] + [0])
    if host:
        hd = data.cpu().numpy().view(dtype)
        ho = offsets.cpu().numpy()
        if longest <= 65534:
            hw, hr = p.find_packed16_packed(hd, ho)
            assert (hw.view(np.int64)[:nw] == w[:nw].cpu().numpy()).all() and (hr == g16).all(), ("host16", what)
        if longest <= 256:
            hw, hr = p.find_packed8_packed(hd, ho)
            assert (hw.view(np.int64)[:nw] == w[:nw].cpu().numpy()).all() and (hr == g8).all(), ("host8", what)
    return s, e


def oracle_find_from(o, h, c):
    if c < 0:
        return (-1, -1)
    try:
        f, s, e = o.find(h, start=int(c))
    except RuntimeError:  # the reference would throw: no oracle answer for this cursor
        return None
    return (s, e) if f else (-1, -1)


def check_cursors(p, o, rows, dtype, lead=5, trail=7, junk=None, seed=0, oracle_rows=400, what=""):
    """find_next_packed for cursors -1, 0, random, len, len + 1, len + 9 (each for every row, then mixed) against
    find_next_batch on the same rows at a fixed stride, and against the oracle on up to oracle_rows rows."""
    import torch
    from needle_amd.pattern import Pattern, unpack_bitmap
    n = len(rows)
    rng = np.random.default_rng(seed)
    lens = np.array([len(r) for r in rows], np.int64)
    data, offsets = device_packed(rows, dtype, lead, trail, junk)
    rt, lt, ovf = Pattern.rows_from_packed(data, offsets)
    kinds = {"-1": np.full(n, -1), "0": np.zeros(n), "random": rng.integers(0, lens + 1), "len": lens, "len+1": lens + 1, "len+9": lens + 9}
    kinds["mixed"] = np.choose(rng.integers(0, 6, n), [kinds[k] for k in ("-1", "0", "random", "len", "len+1", "len+9")])
    idx = np.arange(n) if n <= oracle_rows else rng.choice(n, oracle_rows, replace=False)
    for kind, cur in kinds.items():
        c = torch.from_numpy(cur.astype(np.int32)).cuda()
        w, s, e = p.find_next_packed(data, offsets, c)
        xw, xs, xe = p.find_next_batch(rt, c, lt)
        torch.cuda.synchronize()
        nw = (n + 63) // 64
        assert torch.equal(w[:nw], xw[:nw]) and torch.equal(s, xs) and torch.equal(e, xe), ("fixed stride", kind, what)
        gs, ge, gf = s.cpu().numpy(), e.cpu().numpy(), unpack_bitmap(w, n)
        for i in idx:
            want = oracle_find_from(o, np.asarray(rows[i]), cur[i])
            if want is None:
                continue
            assert (int(gs[i]), int(ge[i])) == want, (what, kind, i, int(lens[i]), int(cur[i]), int(gs[i]), int(ge[i]), want)
            assert bool(gf[i]) == (want[1] >= 0 and cur[i] >= 0), (what, kind, i)
    assert int(ovf.item()) == 0


def check_enumeration(p, rows, dtype, what=""):
    """Feeding `end` back as the next cursor, each row stopped under the find-all rule (an empty match, or one that does not end
    beyond its cursor, ends the row), gives find_all_packed's matches (non-nullable patterns)."""
    import torch
    n = len(rows)
    data, offsets = device_packed(rows, dtype, 3, 3)
    off, fs, fe = p.find_all_packed(data, offsets)
    got = [[] for _ in range(n)]
    cur = torch.zeros(n, dtype=torch.int32, device="cuda")
    for _ in range(10000):
        _, s, e = p.find_next_packed(data, offsets, cur)
        sc, ec, cc = s.cpu().numpy(), e.cpu().numpy(), cur.cpu().numpy()
        nxt = np.full(n, -1, np.int32)
        for i in np.nonzero((cc >= 0) & (ec >= 0))[0]:
            got[i].append((int(sc[i]), int(ec[i])))
            if ec[i] != sc[i] and ec[i] > cc[i]:
                nxt[i] = ec[i]
        if (nxt < 0).all():
            break
        cur = torch.from_numpy(nxt).cuda()
    off = off.cpu().numpy()
    fs, fe = fs.cpu().numpy(), fe.cpu().numpy()
    for i in range(n):
        w = list(zip(fs[off[i]:off[i + 1]].tolist(), fe[off[i]:off[i + 1]].tolist()))
        assert got[i] == w, (what, i, got[i][:5], w[:5])


def _script_alphabet():
    from needle_amd import workload as W
    al = [ord(ch) for ch in "ab 09."]
    for a, b in W.SCRIPT_RANGES[:12]:
        al += [a, (a + b) // 2, b]
    return al


# (regex, char width, alphabet, planted words, junk)
PATTERNS = [
    ("abc|xyz", 1, "abcxyz ", ["abc", "xyz"], "abc"),                                                    # fixed length
    ("[0-9]+", 1, "abcxyz 0123456789", [], "0123"),                                                     # packed functions, backward walk
    ("a.*b", 1, "abx\n", [], "ab"),                                                                     # backward walk over the whole row
    ("a*", 1, "aab", [], "aa"),                                                                         # nullable, root-accepting
    ("x?", 1, "xy", [], "x"),
    ("Sherlock|Holmes|Watson|Irene|Adler|John|Baker", 1, "SherlockHmsWatnIdJB ", ["Sherlock", "Holmes", "Baker"], "Holmes"),  # pair table
    ("[α-ω]{2}[α-ω]*", 2, "ab αβω￿", ["αβγ"], "αβγ"),
    ("[a-z一-丠]+[0-9]|ЖЗ+", 2, "az9一丐丰ЖЗ ", ["一丁x7", "ЖЗЗ"], "一a1"),
]


# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("regex,cw,alphabet,plants,junk", PATTERNS)
def test_forms_and_cursors(regex, cw, alphabet, plants, junk):
    p, o = compiled(regex)
    dtype = np.uint8 if cw == 1 else np.uint16
    rng = np.random.default_rng(11 + len(regex))
    al = [ord(ch) for ch in alphabet]
    jk = [ord(ch) for ch in junk]
    rows = layout_rows(rng, al, plants, n=700, dtype=dtype)
    check_forms(p, rows, dtype, lead=5, trail=7, junk=jk, what="lead 5 trail 7")
    check_forms(p, rows, dtype, lead=133, trail=0, junk=jk, what="offsets[0] > 0, last row at the tensor's end")
    for n in (1, 63, 65):
        check_forms(p, rows[48:48 + n], dtype, lead=3, trail=5, junk=jk, what="n_rows %d" % n)
    check_cursors(p, o, rows, dtype, lead=5, trail=7, junk=jk, seed=len(regex), what=regex)
    check_cursors(p, o, rows[:130], dtype, lead=0, trail=0, junk=jk, seed=1, what=(regex, "no lead"))
    if regex not in ("a*", "x?"):
        check_enumeration(p, rows[:300], dtype, what=regex)


@pytest.mark.gpu
def test_dictionaries_lengths_form_and_compressed_automaton():
    """The 300-keyword lengths-form dictionary (LDS table) and a 1000-keyword 6..8-char dictionary (the compressed automaton of
    C3-sparse), 8- and 16-bit rows."""
    from needle_amd import workload as W
    rng = np.random.default_rng(5)
    for words, modes in ((W.keywords(300), (1, 2, 4)), (W.keywords(1000, min_len=6, max_len=8), (6,))):
        p, o = compiled("|".join(words))
        assert p.info()["kernel_mode"]["forwards"] in modes, (len(words), p.info()["kernel_mode"])
        rows = layout_rows(rng, [ord(ch) for ch in "abcdefghijklmnopqrstuvwxyz "], words, n=1200, max_len=200)
        check_forms(p, rows, np.uint8, lead=11, trail=11, junk=[ord(ch) for ch in words[0]], what=len(words))
        check_cursors(p, o, rows, np.uint8, lead=11, trail=11, seed=2, what=len(words))
        check_enumeration(p, rows[:400], np.uint8, what=len(words))
        rows16 = [r.astype(np.uint16) for r in rows[:500]]
        check_forms(p, rows16, np.uint16, lead=6, trail=0, junk=[ord(ch) for ch in words[1]], what=(len(words), 16))
        check_cursors(p, o, rows16, np.uint16, lead=6, trail=0, seed=3, oracle_rows=200, what=(len(words), 16))


@pytest.mark.gpu
def test_c5_class_regex():
    from needle_amd import workload as W
    p, o = compiled(W.script_regex())
    al = _script_alphabet()
    rows = layout_rows(np.random.default_rng(8), al, [], n=900, max_len=150, dtype=np.uint16)
    check_forms(p, rows, np.uint16, lead=3, trail=1, junk=al[6:12], what="c5")
    check_cursors(p, o, rows, np.uint16, lead=3, trail=1, seed=4, what="c5")
    check_enumeration(p, rows[:300], np.uint16, what="c5")


@pytest.mark.gpu
def test_escapes_on_long_rows():
    """Rows of 300 and 70 000 chars with matches on both sides of the 256 / 65 534 limits, among short rows: the escapes appear
    exactly on the rows whose match ends past the limit, the flag is raised, everything else is exact."""
    letters = np.array([ord(ch) for ch in "abdxy "], np.uint8)  # (no match of either pattern but the planted one)
    rng = np.random.default_rng(29)

    def row(n, at):
        r = rng.choice(letters, n).astype(np.uint8)
        if at is not None:  # abc|xyz ends at + 3, [0-9]+ at + 6
            r[at:at + 6] = [ord(ch) for ch in "xyz123"]
        return r
    p, o = compiled("[0-9]+")
    pf, _ = compiled("abc|xyz")
    long_rows = [row(300, 10), row(300, 250), row(300, 252), row(300, 254), row(300, 290), row(300, None), row(260, 254),
                 row(256, 250), row(70000, 100), row(70000, 65528), row(70000, 65530), row(70000, 65532), row(70000, 69000), row(70000, None)]
    short = layout_rows(rng, [ord(ch) for ch in "abc 019"], [], n=300, max_len=60)
    rows = list(short)
    for k, r in enumerate(long_rows):
        rows.insert(5 + 19 * k, r)
    for pat in (p, pf):
        s, e = check_forms(pat, rows, np.uint8, lead=7, trail=5, junk=[ord("9")], what="long among short")
        assert (e > 256).any() and (e > 65534).any() and ((e >= 0) & (e <= 256)).any()
        check_forms(pat, long_rows, np.uint8, lead=1, trail=0, junk=[ord("9")], what="long rows only")
        check_forms(pat, [r.astype(np.uint16) for r in long_rows], np.uint16, lead=1, trail=3, junk=[ord("9")], what="long rows, 16-bit")
        check_forms(pat, short, np.uint8, lead=1, trail=3, junk=[ord("9")], what="no escapes")
    check_cursors(p, o, rows, np.uint8, lead=7, trail=5, junk=[ord("9")], seed=9, what="long rows")


@pytest.mark.gpu
def test_host_entries_chunked():
    """The _host entries in several chunks (NEEDLE_HOST_CHUNK_BYTES in a child process): offsets[0] > 0, chunk borders inside
    groups of short rows, equal to the device entries."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    child = r'''
import sys
sys.path.insert(0, "."); sys.path.insert(0, "tests")
import numpy as np, torch
import test_gpu_find_packed_forms as T
from test_gpu_configs import compiled
from test_gpu_packed_dev import device_packed, layout_rows
p, o = compiled("[0-9]+")
rows = layout_rows(np.random.default_rng(3), [ord(ch) for ch in "abc 0123"], [], n=3000, max_len=200)
T.check_forms(p, rows, np.uint8, lead=17, trail=3, junk=[ord("5")], what="chunked host")
T.check_forms(p, [r.astype(np.uint16) for r in rows], np.uint16, lead=2, trail=0, junk=[ord("5")], what="chunked host 16")
# needle_{find,contained_in,matches}_packed_host on the same host arrays against the oracle: as the rows stand (one length class, many
# chunks), and with one 5 000-char row among them (the padded rows exceed 4x the text + 64 KiB: length classes, each of them chunked)
from needle_amd.pattern import unpack_bitmap
want = [(o.find(s), o.matches(s)) for s in (r.tobytes().decode("latin-1") for r in rows)]
long_row = np.random.default_rng(5).choice(np.array([ord(ch) for ch in "abc 0123"], np.uint8), 5000)
long_want = (o.find(long_row.tobytes().decode("latin-1")), o.matches(long_row.tobytes().decode("latin-1")))
for rs, wt in ((rows, want), (rows[:1234] + [long_row] + rows[1234:], want[:1234] + [long_want] + want[1234:])):
    for dtype in (np.uint8, np.uint16):
        data, offsets = device_packed([r.astype(dtype) for r in rs], dtype, 17, 3, [ord("5")])
        hd, ho = data.cpu().numpy().view(dtype), offsets.cpu().numpy()
        fw, fs, fe = p.find_packed(hd, ho)
        got, cb, mb = (unpack_bitmap(w, len(rs)) for w in (fw, p.contained_in_packed(hd, ho), p.matches_packed(hd, ho)))
        for i, ((found, st, en), full) in enumerate(wt):
            assert got[i] == found and cb[i] == found and mb[i] == full, (i, dtype)
            assert (fs[i], fe[i]) == ((st, en) if found else (-1, -1)), (i, dtype)
print("HOST-CHUNKED-OK")
'''
    r = subprocess.run([sys.executable, "-c", child], env=dict(os.environ, NEEDLE_HOST_CHUNK_BYTES="20000"), capture_output=True, text=True,
                       timeout=600, cwd=root)
    assert "HOST-CHUNKED-OK" in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]


@pytest.mark.gpu
def test_non_default_stream_and_out():
    import torch
    from needle_amd.pattern import Pattern
    p, o = compiled("[0-9]+")
    rows = layout_rows(np.random.default_rng(31), [ord(ch) for ch in "abc 0123"], [], n=5000, max_len=300)
    n = len(rows)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        data, offsets = device_packed(rows, np.uint8, 3, 3, [ord("5")])
        w, st, en = p.find_packed(data, offsets, stream=s.cuda_stream)
        w16, r16, o16 = p.find_packed16_packed(data, offsets, stream=s.cuda_stream)
        w8, r8, o8 = p.find_packed8_packed(data, offsets, stream=s.cuda_stream)
        cur = torch.zeros(n, dtype=torch.int32, device="cuda")
        cw, cs, ce = p.find_next_packed(data, offsets, cur, stream=s.cuda_stream)
    s.synchronize()
    se, ee = st.cpu().numpy(), en.cpu().numpy()
    assert torch.equal(w16, w) and torch.equal(w8, w) and torch.equal(cw, w) and torch.equal(cs, st) and torch.equal(ce, en)
    assert (r16.cpu().numpy().view(np.uint32) == pack16_expected(se, ee)).all()
    assert (r8.cpu().numpy().view(np.uint16) == pack8_expected(se, ee)).all()
    assert int(o16.item()) == 0 and int(o8.item()) == int((ee > 256).any())
    # out=: caller-owned buffers, the overflow flag zeroed by the caller
    nw = (n + 63) // 64
    bm = torch.full((nw,), -1, dtype=torch.int64, device="cuda")
    res = torch.empty(n, dtype=torch.int16, device="cuda")
    flag = torch.zeros(1, dtype=torch.int32, device="cuda")
    got = p.find_packed8_packed(data, offsets, out=(bm, res, flag))
    torch.cuda.synchronize()
    assert got[0] is bm and got[1] is res and got[2] is flag
    assert torch.equal(bm, w) and torch.equal(res, r8) and int(flag.item()) == int(o8.item())
    s_, e_, over = Pattern.unpack8_packed(res.cpu().numpy())
    fits = ee <= 256
    assert (s_[fits] == se[fits]).all() and (e_[fits] == ee[fits]).all() and (over == ~fits).all()
    s_, e_, over = Pattern.unpack16_packed(r16.cpu().numpy())
    assert (s_ == se).all() and (e_ == ee).all() and not over.any()


@pytest.mark.gpu
def test_ten_million_ragged_rows_packed8():
    """10^7 rows of lengths uniform in [1, 256] (bench.py's c3 rows, packed): find_packed8_packed equals the int32 entry packed on the
    device, and the 16-bit form equals it too."""
    import torch
    from needle_amd import workload as W
    n = 10_000_000
    dev = torch.device("cuda")
    lens = (torch.arange(n, device=dev, dtype=torch.int64) * 2654435761 % 256 + 1)
    offsets = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    offsets[1:] = torch.cumsum(lens, 0)
    col = torch.arange(256, device=dev)[None, :]
    words = W.keywords(1000)
    p, o = compiled("|".join(words))
    data = torch.empty(int(offsets[-1].item()), dtype=torch.uint8, device=dev)
    for s in range(0, n, 1 << 20):
        k = min(1 << 20, n - s)
        rows = W.keyword_batch(torch, words, s, k, 256, device=dev)
        data[int(offsets[s].item()):int(offsets[s + k].item())] = rows[col < lens[s:s + k, None]]
    w, st, en = p.find_packed(data, offsets)
    w8, r8, o8 = p.find_packed8_packed(data, offsets)
    w16, r16, o16 = p.find_packed16_packed(data, offsets)
    # pack8 of the int32 results on the device
    ln = en - st
    held = torch.where(ln > 255, torch.full_like(ln, 0xFFFE), (st & 0xFF) | (ln << 8))
    want8 = torch.where(en < 0, torch.full_like(en, 0xFFFF), held).to(torch.int32)
    want16 = torch.where(en < 0, torch.full_like(en, -1), (st & 0xFFFF) | (en << 16))
    torch.cuda.synchronize()
    assert torch.equal(w8, w) and torch.equal(w16, w)
    assert torch.equal(r8.to(torch.int32) & 0xFFFF, want8) and int(o8.item()) == 0
    assert torch.equal(r16, want16) and int(o16.item()) == 0
    assert int(w.ne(0).sum().item()) > 0
