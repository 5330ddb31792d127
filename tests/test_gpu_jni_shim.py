"""bindings/jni/needle_jni.c on the GPU, through the fake JNIEnv of tests/jni/ (a stand-in jni.h, NOT a JVM's table layout: nothing here is
ever loaded by a JVM).  One process; libneedle_jni_fake.so is loaded with ctypes; patterns are compiled through the `compile` native.

Every result is compared with a reference that does not go through the shim: the oracle (oracle/needle_walk.c on the tables of
DFACompiler.compile, as tests/test_gpu_fuzz.py uses it) and the plain-Python references of tests/utf8_cases.py, tests/gather_cases.py,
tests/pattern_set_cases.py and tests/set_spans_cases.py -- never the ctypes host entry alone.

The fake hands out COPIES of every array between sentinels, and the output arrays are exactly as long as the contract says: a result
released with JNI_ABORT (or not at all) is invisible here, an overrun by one element is a recorded fault.  After every call: no
outstanding pin, an empty fault log, every input byte-identical."""
import json
import os
import random

import numpy as np
import pytest

import jni_shim_cases as J
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

OK, ERR_INVALID, ERR_UNSUPPORTED = 0, 1, 4
ROW_COUNTS = [0, 1, 63, 64, 65, 130]
DICTIONARY = "cat|dog|mouse|кот|собака|мышь"  # two scripts
PATTERNS = ["[0-9]+", "Sherlock|Holmes|Watson", "(ab|cd)+e?", "x*", DICTIONARY, "[α-ω]{2}[α-ω]*"]
PIECES = ["0", "42", "2024", "Sherlock", "Holmes", "Watson", "ab", "cd", "abcde", "cdabe", "x", "xxx", "cat", "dog", "mouse", "кот", "собака", "мышь",
          "αβ", "ωωω", "α", " ", "_", "e", "é", "Ж", "中", "耀", "￿", "y", "Z"]
PIECES8 = [p for p in PIECES if all(ord(c) < 256 for c in p)]
GARBAGE = 0x5A


@pytest.fixture(scope="module")
def fake(tmp_path_factory):
    f = J.Fake(J.build_fake(tmp_path_factory.mktemp("jni_fake_gpu"))[0])
    yield f
    for h, _ in _patterns.values():
        f.call("destroyPattern", h)
    _patterns.clear()
    f.reset()
    import torch
    print("\non %s, natives called through the fake JNIEnv: " % torch.cuda.get_device_name(0) + ", ".join("%s %d" % kv for kv in sorted(CALLS.items())))


@pytest.fixture(autouse=True)
def fresh_objects(fake):
    """Every test starts with an empty fake JVM (pattern handles are the library's and stay)."""
    yield
    fake.reset()


# ---- the shim's side ---------------------------------------------------------------------------------------------------------------
_patterns = {}
CALLS = {}  # native -> calls made by this module, printed when it is done


def shim_pattern(fake, regex, flags=0):
    """(handle made by the `compile` native, the oracle of the same regex) -- once per process."""
    if (regex, flags) not in _patterns:
        from test_compile_matches_txt import oracle_for
        out = fake.array("long", [0])
        assert call(fake, "compile", fake.array("char", J.u16(regex)), flags, out) == OK, regex
        _patterns[regex, flags] = (int(fake.read(out)[0]), oracle_for(regex, flags)[0])
    return _patterns[regex, flags]


def call(fake, name, *args, inputs=(), buffers=()):
    """The native; then: nothing pinned, no fault, the input arrays and direct buffers byte-identical."""
    before = [fake.read_bytes(h) for h in inputs]
    kept = [b.copy() for b in buffers]
    rc = fake.call(name, *args)
    CALLS[name] = CALLS.get(name, 0) + 1
    fake.assert_clean(name)
    for h, b in zip(inputs, before):
        assert fake.read_bytes(h) == b, (name, "an input array was changed")
    for a, b in zip(buffers, kept):
        assert (a == b).all(), (name, "an input buffer was changed")
    return rc


def out_array(fake, kind, n):
    """An output array of exactly n elements, filled with garbage."""
    return fake.array(kind, np.frombuffer(bytes([GARBAGE]) * (n * J.ITEM[kind]), dtype=J.KINDS[kind][1]))


def garbage_of(kind):
    return np.frombuffer(bytes([GARBAGE]) * J.ITEM[kind], dtype=J.KINDS[kind][1])[0]


def bits(words, n):
    return np.unpackbits(np.ascontiguousarray(words).view(np.uint8), bitorder="little")[:n].astype(bool)


# ---- rows --------------------------------------------------------------------------------------------------------------------------
def make_rows(n, seed, wide=True, max_len=70, long_row=False):
    """n rows of 0 .. max_len chars made of PIECES (UTF-16 rows: 0x00E9, 0x0416, 0x4E2D, 0x8000, 0xFFFF among them); some rows empty, the
    last row empty; with long_row one more row of 9000 chars in the middle."""
    rng = random.Random(seed)
    pieces, dtype = (PIECES, np.uint16) if wide else (PIECES8, np.uint8)
    rows = []
    for r in range(n):
        want = 0 if r == n - 1 or r % 11 == 3 else rng.randrange(0, max_len + 1)
        text = ""
        while len(text) < want:
            text += rng.choice(pieces)
        rows.append(np.array([ord(c) for c in text[:want]], dtype=dtype))
    if long_row:
        text = "".join(rng.choice(pieces) for _ in range(9000))[:9000]
        rows.insert(n // 2, np.array([ord(c) for c in text], dtype=dtype))
    return rows


def pack(rows, dtype=np.uint16):
    off = np.zeros(len(rows) + 1, np.int64)
    off[1:] = np.cumsum([len(r) for r in rows])
    return (np.concatenate(rows).astype(dtype) if len(rows) and off[-1] else np.zeros(0, dtype)), off


def pad(rows, stride, dtype):
    a = np.zeros((len(rows), stride), dtype=dtype)
    for i, r in enumerate(rows):
        a[i, :len(r)] = r
    return a, np.array([len(r) for r in rows], dtype=np.uint32)


def oracle_find(o, rows, dtype=np.uint16):
    """(found, start, end) per row from the oracle's batch_find; rows bucketed so that one 9000-char row does not pad all."""
    n = len(rows)
    f, s, e = np.zeros(n, bool), np.full(n, -1, np.int32), np.full(n, -1, np.int32)
    short = [i for i, r in enumerate(rows) if len(r) <= 70]
    for idx in (short, [i for i in range(n) if len(rows[i]) > 70]):
        if idx:
            p, L = pad([rows[i] for i in idx], max(1, max(len(rows[i]) for i in idx)), dtype)
            f[idx], s[idx], e[idx] = o.batch_find(p, L, threads=4)
    return f, s, e


def oracle_bits(o, rows, op, dtype=np.uint16):
    n = len(rows)
    out = np.zeros(n, bool)
    short = [i for i, r in enumerate(rows) if len(r) <= 70]
    for idx in (short, [i for i in range(n) if len(rows[i]) > 70]):
        if idx:
            p, L = pad([rows[i] for i in idx], max(1, max(len(rows[i]) for i in idx)), dtype)
            out[idx] = (o.batch_matches if op == 0 else o.batch_contained_in)(p, L, threads=4)
    return out


def oracle_find_all(o, rows):
    return [o.find_all(np.ascontiguousarray(r)) for r in rows]


def fixed_args(fake, rows, cw, with_lengths, stride=72, row_len=70):
    """The direct buffers of a fixed-stride batch: (args rows .. lengths, the numpy arrays behind them, the rows as the native sees them)."""
    dtype = np.uint8 if cw == 1 else np.uint16
    a, L = pad(rows, stride, dtype)
    mem = a if a.size else np.zeros(8, dtype)  # (0 rows: still a buffer)
    if with_lengths:
        lm = L if L.size else np.zeros(4, np.uint32)
        return (fake.buffer(mem), cw, len(rows), stride, row_len, fake.buffer(lm)), [mem, lm], rows
    # every row is row_len chars: the padding zeros are text
    return (fake.buffer(mem), cw, len(rows), stride, row_len, None), [mem], [a[i, :row_len] for i in range(len(rows))]


# (rows, stride, row_len, with a 9000-char row): 0 .. 130 rows of at most 70 chars, and 66 rows of which one has 9000
FIXED_BATCHES = [(n, 72, 70, False) for n in ROW_COUNTS] + [(65, 9008, 9000, True)]


# ---- find / matches / containedIn --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("regex", PATTERNS)
def test_fixed_stride_natives_against_the_oracle(fake, regex):
    """matchesHost / containedInHost / findHost and scanHostMulti (ops 0 / 1 / 2 on a one-device multiCreate) over direct buffers, char width
    1 and 2, with and without lengths, 0 .. 130 rows of at most 70 chars and one batch at stride 9008 holding a 9000-char row: bitmap words and start / end equal to the oracle's batch_matches / batch_contained_in /
    batch_find; findPacked16Host / findPacked8Host / findCompactHost decoded by the header's packing rules, against batch_find."""
    h, o = shim_pattern(fake, regex)
    m_out = fake.array("long", [0])
    assert call(fake, "multiCreate", fake.array("int", [0]), 0, m_out) == OK
    multi = int(fake.read(m_out)[0])
    try:
        fixed_stride_natives(fake, regex, h, o, multi)
    finally:
        fake.call("multiDestroy", multi)


def fixed_stride_natives(fake, regex, h, o, multi):
    for cw in (1, 2):
        dtype = np.uint8 if cw == 1 else np.uint16
        for with_lengths in (True, False):
            for n, stride, row_len, long_row in FIXED_BATCHES:
                rows = make_rows(n, 100 * cw + n, wide=cw == 2, long_row=long_row)
                n = len(rows)
                view, bufs, seen = fixed_args(fake, rows, cw, with_lengths, stride, row_len)
                words = (n + 63) // 64
                what = (regex, "cw", cw, "lengths", with_lengths, "rows", n, "stride", stride)
                sp, L = pad(seen, stride, dtype)
                want = {0: o.batch_matches(sp, L, threads=4), 1: o.batch_contained_in(sp, L, threads=4)} if n else {0: np.zeros(0, bool), 1: np.zeros(0, bool)}
                wf, ws, we = o.batch_find(sp, L, threads=4) if n else (np.zeros(0, bool), np.zeros(0, np.int32), np.zeros(0, np.int32))
                for op, name in ((0, "matchesHost"), (1, "containedInHost")):
                    bm = out_array(fake, "long", words)
                    assert call(fake, name, h, *view, bm, buffers=bufs) == OK, what
                    assert (bits(fake.read(bm), n) == want[op]).all(), (what, name, "oracle.batch_matches / batch_contained_in")
                    bm = out_array(fake, "long", words)
                    assert call(fake, "scanHostMulti", multi, h, op, *view, bm, None, None, buffers=bufs) == OK, what
                    assert (bits(fake.read(bm), n) == want[op]).all(), (what, "scanHostMulti", op, "oracle.batch_matches / batch_contained_in")
                for name, lead in (("findHost", (h,)), ("scanHostMulti", (multi, h, 2))):
                    bm, st, en = out_array(fake, "long", words), out_array(fake, "int", n), out_array(fake, "int", n)
                    assert call(fake, name, *lead, *view, bm, st, en, buffers=bufs) == OK, what
                    assert (bits(fake.read(bm), n) == wf).all(), (what, name, "oracle.batch_find: found")
                    assert (fake.read(st) == ws).all() and (fake.read(en) == we).all(), (what, name, "oracle.batch_find: start / end")
                # one int per row: start | end << 16, 0xFFFFFFFF no match
                bm, se = out_array(fake, "long", words), out_array(fake, "int", n)
                assert call(fake, "findPacked16Host", h, *view, bm, se, buffers=bufs) == OK, what
                v = fake.read(se).view(np.uint32)
                lo, hi = (v & 0xFFFF).astype(np.int64), (v >> 16).astype(np.int64)
                assert (bits(fake.read(bm), n) == wf).all() and (np.where(v == 0xFFFFFFFF, -1, lo) == ws).all() and (np.where(v == 0xFFFFFFFF, -1, hi) == we).all(), \
                    (what, "findPacked16Host", "oracle.batch_find")
                # one short per row: NEEDLE_UNPACK8_START / _END
                bm, sl = out_array(fake, "long", words), out_array(fake, "short", n)
                rc = call(fake, "findPacked8Host", h, *view, bm, sl, buffers=bufs)
                if stride > 256:  # refused before any device call, nothing written
                    assert rc == ERR_UNSUPPORTED and (fake.read(sl) == garbage_of("short")).all() and (fake.read(bm) == garbage_of("long")).all(), what
                else:
                    assert rc == OK, what
                    x = fake.read(sl).view(np.uint16).astype(np.int64)
                    s8 = np.where(x == 0xFFFF, -1, np.where(x == 0xFFFE, 0, x & 0xFF))
                    e8 = np.where(x == 0xFFFF, -1, np.where(x == 0xFFFE, 256, (x & 0xFF) + (x >> 8)))
                    assert (bits(fake.read(bm), n) == wf).all() and (s8 == ws).all() and (e8 == we).all(), (what, "findPacked8Host", "oracle.batch_find")
                # the matched rows only: records (row, start | end << 16), room for all, for one fewer, for none
                hit = np.nonzero(wf)[0]
                for cap in sorted({len(hit), max(len(hit) - 1, 0), 0}):
                    bm, nm = out_array(fake, "long", words), out_array(fake, "long", 1)
                    rec = out_array(fake, "int", 2 * cap) if cap else None
                    assert call(fake, "findCompactHost", h, *view, bm, rec, nm, buffers=bufs) == OK, what
                    assert int(fake.read(nm)[0]) == len(hit) and (bits(fake.read(bm), n) == wf).all(), (what, "findCompactHost", "oracle.batch_find")
                    if cap:
                        r = fake.read(rec).view(np.uint32).reshape(cap, 2)
                        assert (r[:, 0] == hit[:cap]).all() and ((r[:, 1] & 0xFFFF) == ws[hit[:cap]]).all() and ((r[:, 1] >> 16) == we[hit[:cap]]).all(), \
                            (what, "findCompactHost records", "oracle.batch_find")


@pytest.mark.parametrize("regex", PATTERNS)
def test_packed_host_ops_against_the_oracle(fake, regex):
    """packedHost ops 0 / 1 / 2 (the native behind findBatch(String[])) and both compact forms over char[] + offsets: 0 .. 130 rows of 0 .. 70
    chars, one batch with a 9000-char row; against the oracle's batch_matches / batch_contained_in / batch_find."""
    h, o = shim_pattern(fake, regex)
    for n, long_row in [(n, False) for n in ROW_COUNTS] + [(65, True)]:
        rows = make_rows(n, 7 + n, long_row=long_row)
        n = len(rows)
        data_np, off_np = pack(rows)
        data, off = fake.array("char", data_np), fake.array("long", off_np)
        words, what = (n + 63) // 64, (regex, "rows", n, "long row", long_row)
        for op in (0, 1):
            bm = out_array(fake, "long", words)
            assert call(fake, "packedHost", h, op, data, off, bm, None, None, inputs=(data, off)) == OK, what
            assert (bits(fake.read(bm), n) == oracle_bits(o, rows, op)).all(), (what, op, "oracle.batch_matches / batch_contained_in")
        wf, ws, we = oracle_find(o, rows)
        bm, st, en = out_array(fake, "long", words), out_array(fake, "int", n), out_array(fake, "int", n)
        assert call(fake, "packedHost", h, 2, data, off, bm, st, en, inputs=(data, off)) == OK, what
        assert (bits(fake.read(bm), n) == wf).all() and (fake.read(st) == ws).all() and (fake.read(en) == we).all(), (what, "oracle.batch_find")
        bm, se = out_array(fake, "long", words), out_array(fake, "int", n)
        assert call(fake, "findPacked16PackedHost", h, data, off, bm, se, inputs=(data, off)) == OK, what
        v = fake.read(se).view(np.uint32)
        assert (bits(fake.read(bm), n) == wf).all() and (np.where(v == 0xFFFFFFFF, -1, (v & 0xFFFF).astype(np.int64)) == ws).all() and \
            (np.where(v == 0xFFFFFFFF, -1, (v >> 16).astype(np.int64)) == we).all(), (what, "findPacked16PackedHost", "oracle.batch_find")
        bm, sl = out_array(fake, "long", words), out_array(fake, "short", n)
        rc = call(fake, "findPacked8PackedHost", h, data, off, bm, sl, inputs=(data, off))
        if long_row:  # a row over 256 chars: refused before any device call, nothing written
            assert rc == ERR_UNSUPPORTED, what
            assert (fake.read(sl) == garbage_of("short")).all() and (fake.read(bm) == garbage_of("long")).all(), what
        else:
            assert rc == OK, what
            x = fake.read(sl).view(np.uint16).astype(np.int64)
            assert (np.where(x == 0xFFFF, -1, np.where(x == 0xFFFE, 0, x & 0xFF)) == ws).all(), (what, "findPacked8PackedHost", "oracle.batch_find")
            assert (np.where(x == 0xFFFF, -1, np.where(x == 0xFFFE, 256, (x & 0xFF) + (x >> 8))) == we).all(), (what, "findPacked8PackedHost", "oracle.batch_find")


def test_compact_forms_refuse_rows_beyond_their_limit(fake):
    """A row of 257 resp. 65 535 chars: NEEDLE_ERR_UNSUPPORTED from both pairs of findPacked16... / findPacked8..., outputs untouched."""
    h, _ = shim_pattern(fake, "[0-9]+")
    for limit, names in ((256, ("findPacked8Host", "findPacked8PackedHost")), (65534, ("findPacked16Host", "findPacked16PackedHost"))):
        kind = "short" if limit == 256 else "int"
        row = np.full(limit + 1, ord("7"), np.uint16)
        rows = [np.array([ord("1")], np.uint16), row]
        data_np, off_np = pack(rows)
        data, off = fake.array("char", data_np), fake.array("long", off_np)
        bm, res = out_array(fake, "long", 1), out_array(fake, kind, 2)
        assert call(fake, names[1], h, data, off, bm, res, inputs=(data, off)) == ERR_UNSUPPORTED, names[1]
        assert (fake.read(res) == garbage_of(kind)).all()
        a = np.zeros((2, limit + 1), np.uint16)
        a[1] = row
        bm, res = out_array(fake, "long", 1), out_array(fake, kind, 2)
        assert call(fake, names[0], h, fake.buffer(a), 2, 2, limit + 1, limit + 1, None, bm, res) == ERR_UNSUPPORTED, names[0]
        assert (fake.read(res) == garbage_of(kind)).all()
        # ... and at the limit itself both answer (the oracle: one match, the whole row)
        rows = [np.full(limit, ord("7"), np.uint16)]
        data_np, off_np = pack(rows)
        data, off = fake.array("char", data_np), fake.array("long", off_np)
        bm, res = out_array(fake, "long", 1), out_array(fake, kind, 1)
        assert call(fake, names[1], h, data, off, bm, res, inputs=(data, off)) == OK
        x = int(fake.read(res).view(np.uint16 if limit == 256 else np.uint32)[0])
        assert x == (0xFFFE if limit == 256 else (limit << 16)), (names[1], hex(x), "oracle: (0, %d)" % limit)


# ---- find-all ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("regex", PATTERNS)
def test_find_all_natives_against_the_oracle(fake, regex):
    """findAllHost, findAllPacked16Host, findAllCsrHost (direct buffers) and findAllPackedHost (char[] + offsets) against oracle.find_all:
    slots, counts and `more`; start / end null (count only); capacity exact and one short of the total; 0 .. 130 rows of at most 70 chars and
    one batch with a 9000-char row."""
    h, o = shim_pattern(fake, regex)
    for n, stride, row_len, long_row in FIXED_BATCHES:
        for cw in (1, 2):
            rows = make_rows(n, 31 * cw + n, wide=cw == 2, long_row=long_row)
            n = len(rows)
            want = oracle_find_all(o, rows)
            counts = np.array([len(w) for w in want], np.int64)
            total, what = int(counts.sum()), (regex, "cw", cw, "rows", n, "stride", stride)
            flat_s = np.array([s for w in want for s, _ in w], np.int32)
            flat_e = np.array([e for w in want for _, e in w], np.int32)
            view, bufs, _ = fixed_args(fake, rows, cw, True, stride, row_len)
            for k in (3, 40):  # slots per row: fewer than some rows have, more than any row has
                cn, st, en, more = out_array(fake, "int", n), out_array(fake, "int", n * k), out_array(fake, "int", n * k), out_array(fake, "int", 1)
                assert call(fake, "findAllHost", h, *view, k, cn, st, en, more, buffers=bufs) == OK, what
                got_c, got_s, got_e = fake.read(cn), fake.read(st).reshape(n, k), fake.read(en).reshape(n, k)
                assert (got_c == np.minimum(counts, k)).all() and int(fake.read(more)[0]) == int((counts > k).any()), (what, k, "oracle.find_all: counts / more")
                c16, se, more16 = out_array(fake, "int", n), out_array(fake, "int", n * k), out_array(fake, "int", 1)
                assert call(fake, "findAllPacked16Host", h, *view, k, c16, se, more16, buffers=bufs) == OK, what
                got16 = fake.read(se).view(np.uint32).reshape(n, k)
                assert (fake.read(c16) == got_c).all() and int(fake.read(more16)[0]) == int((counts > k).any()), (what, k, "oracle.find_all: counts / more")
                for r in range(n):
                    w = want[r][:k]
                    assert list(zip(got_s[r, :len(w)].tolist(), got_e[r, :len(w)].tolist())) == w, (what, k, r, "oracle.find_all")
                    assert (got_s[r, len(w):] == -1).all() and (got_e[r, len(w):] == -1).all(), (what, k, r, "slots beyond the count")
                    assert [(int(x & 0xFFFF), int(x >> 16)) for x in got16[r, :len(w)]] == w, (what, k, r, "oracle.find_all, one dword per match")
                    assert (got16[r, len(w):] == 0xFFFFFFFF).all(), (what, k, r, "slots beyond the count")
            if cw == 2:
                data_np, off_np = pack(rows)
                data, off = fake.array("char", data_np), fake.array("long", off_np)
            for name in ("findAllCsrHost", "findAllPackedHost") if cw == 2 else ("findAllCsrHost",):
                for cap in (None, total, total - 1):
                    if cap is not None and cap < 0:
                        continue
                    mo, tt = out_array(fake, "long", n + 1), out_array(fake, "long", 1)
                    st = en = None
                    if cap is not None:
                        st, en = out_array(fake, "int", cap), out_array(fake, "int", cap)
                    if name == "findAllCsrHost":
                        rc = call(fake, name, h, *view, mo, st, en, tt, buffers=bufs)
                    else:
                        rc = call(fake, name, h, data, off, mo, st, en, tt, inputs=(data, off))
                    assert rc == OK, (what, name, cap)
                    assert int(fake.read(tt)[0]) == total, (what, name, cap, "oracle.find_all: total")
                    assert (fake.read(mo) == np.concatenate([[0], np.cumsum(counts)])).all(), (what, name, cap, "oracle.find_all: offsets")
                    if cap == total and total:
                        assert (fake.read(st) == flat_s).all() and (fake.read(en) == flat_e).all(), (what, name, "oracle.find_all")
                    elif cap:  # one short: what is filed is a prefix of the list, the rest of the arrays is as it was
                        gs, ge = fake.read(st), fake.read(en)
                        filed = int(np.nonzero(gs != garbage_of("int"))[0].max()) + 1 if (gs != garbage_of("int")).any() else 0
                        assert (gs[:filed] == flat_s[:filed]).all() and (ge[:filed] == flat_e[:filed]).all() and (ge[filed:] == garbage_of("int")).all(), \
                            (what, name, "capacity one short", "oracle.find_all")


# ---- UTF-8 -------------------------------------------------------------------------------------------------------------------------
def utf8_batches():
    from utf8_cases import alphabet_rows, long_row, random_rows
    every = alphabet_rows()
    yield "a 9000-byte row among 64", random_rows(32, 77, max_len=24) + [long_row(9000, 3)] + random_rows(31, 78, max_len=24) + [b""]
    yield "alphabet rows (every 997th) + random", every[::997] + random_rows(130, 5) + [b""]
    for n in ROW_COUNTS:
        yield "random %d" % n, random_rows(n, 40 + n, max_len=24)[:max(n - 1, 0)] + ([b""] if n else [])


@pytest.mark.parametrize("regex", ["[\u0080-￿]+|A", "�", "[α-ω]{2}[α-ω]*|\x00"])
def test_utf8_natives_against_cpython_and_the_oracle(fake, regex):
    """findAllUtf8PackedHost / containedInUtf8PackedHost on ill-formed and well-formed UTF-8: the rows decoded by CPython's
    bytes.decode("utf-8", "replace"), oracle.find_all / contained_in on those units, the unit positions mapped to bytes by utf8_cases.unit_bytes
    (byte_of_unit's table); `malformed` (utf8_cases.Expected) given and null; one batch holds a 9000-byte row."""
    from utf8_cases import Expected, unit_bytes
    h, o = shim_pattern(fake, regex)
    for label, rows in utf8_batches():
        n, words = len(rows), (len(rows) + 63) // 64
        units = [np.frombuffer(r.decode("utf-8", "replace").encode("utf-16-le", "surrogatepass"), dtype=np.uint16) for r in rows]
        maps = [unit_bytes(r) for r in rows]  # byte_of_unit(r, p) = maps[r][min(p, U)], computed once per row
        want = [[(b[min(s, len(b) - 1)], b[min(e, len(b) - 1)]) for s, e in o.find_all(np.ascontiguousarray(u))] for b, u in zip(maps, units)]
        counts = np.array([len(w) for w in want], np.int64)
        total = int(counts.sum())
        contained = np.array([o.contained_in(np.ascontiguousarray(u)) for u in units], bool)
        bad = np.array(Expected(rows).malformed, bool)
        off_np = np.zeros(n + 1, np.int64)
        off_np[1:] = np.cumsum([len(r) for r in rows])
        data, off = fake.array("byte", np.frombuffer(b"".join(rows), dtype=np.int8)), fake.array("long", off_np)
        for with_malformed in (True, False):
            what = (regex, label, "malformed", with_malformed)
            ml = out_array(fake, "long", words) if with_malformed else None
            bm = out_array(fake, "long", words)
            assert call(fake, "containedInUtf8PackedHost", h, data, off, bm, ml, inputs=(data, off)) == OK, what
            assert (bits(fake.read(bm), n) == contained).all(), (what, "bytes.decode + oracle.contained_in")
            assert ml is None or (bits(fake.read(ml), n) == bad).all(), (what, "utf8_cases.Expected.malformed")
            for cap in (None, total, total - 1):
                if cap is not None and cap < 0:
                    continue
                ml = out_array(fake, "long", words) if with_malformed else None
                mo, tt = out_array(fake, "long", n + 1), out_array(fake, "long", 1)
                st, en = (None, None) if cap is None else (out_array(fake, "int", cap), out_array(fake, "int", cap))
                assert call(fake, "findAllUtf8PackedHost", h, data, off, mo, st, en, tt, ml, inputs=(data, off)) == OK, (what, cap)
                assert int(fake.read(tt)[0]) == total and (fake.read(mo) == np.concatenate([[0], np.cumsum(counts)])).all(), (what, cap, "bytes.decode + oracle.find_all")
                assert ml is None or (bits(fake.read(ml), n) == bad).all(), (what, cap, "utf8_cases.Expected.malformed")
                if cap == total and total:
                    got = list(zip(fake.read(st).tolist(), fake.read(en).tolist()))
                    assert got == [m for w in want for m in w], (what, "bytes.decode + oracle.find_all + utf8_cases.unit_bytes")


# ---- replace, gather ---------------------------------------------------------------------------------------------------------------
def splice(row, matches, repl):
    out, at = [], 0
    for (s, e), r in zip(matches, repl):
        out.append(row[at:s])
        out.append(row[s:e] if r is None else r)
        at = e
    out.append(row[at:])
    return np.concatenate(out).astype(np.uint16)


@pytest.mark.parametrize("regex", PATTERNS)
def test_replace_and_gather_natives_against_python_splices(fake, regex):
    """replaceAllPackedHost against the oracle's match list spliced in Python (a replacement and the empty one); gatherMatchesPackedHost modes
    0 and 1 against gather_cases.gather_ref / split_list_ref of that list; `out` null (sizes only), exact, one short."""
    from gather_cases import gather_ref, split_list_ref
    h, o = shim_pattern(fake, regex)
    for n, long_row in [(n, False) for n in ROW_COUNTS] + [(64, True)]:
        rows = make_rows(n, 900 + n, long_row=long_row)
        n = len(rows)
        lists = oracle_find_all(o, rows)
        data_np, off_np = pack(rows)
        data, off = fake.array("char", data_np), fake.array("long", off_np)
        for repl_text in ("<耀#>", ""):
            repl_np = J.u16(repl_text)
            repl = fake.array("char", repl_np)
            want_rows = [splice(r, m, [repl_np] * len(m)) for r, m in zip(rows, lists)]
            want_text, want_off = pack(want_rows)
            what = (regex, "rows", n, "replacement", repl_text)
            for cap in (None, len(want_text), len(want_text) - 1):
                if cap is not None and cap < 0:
                    continue
                oo, tt = out_array(fake, "long", n + 1), out_array(fake, "long", 1)
                out = None if cap is None else out_array(fake, "char", cap)
                assert call(fake, "replaceAllPackedHost", h, data, off, repl, oo, out, tt, inputs=(data, off, repl)) == OK, (what, cap)
                assert int(fake.read(tt)[0]) == len(want_text) and (fake.read(oo) == want_off).all(), (what, cap, "oracle.find_all spliced in Python: sizes")
                if cap == len(want_text) and cap:
                    assert (fake.read(out) == want_text).all(), (what, "oracle.find_all spliced in Python")
        for mode in (0, 1):
            spans = lists if mode == 0 else split_list_ref(rows, lists)
            per_row = gather_ref(rows, spans)
            parts = [np.asarray(x, np.uint16) for per in per_row for x in per]
            want_text, want_off = pack(parts)
            want_span_off = np.concatenate([[0], np.cumsum([len(p) for p in per_row])]).astype(np.int64)
            what = (regex, "rows", n, "gather mode", mode)
            for span_cap, unit_cap in ((None, None), (len(parts), len(want_text)), (len(parts), len(want_text) - 1)):
                if unit_cap is not None and unit_cap < 0:
                    continue
                so, tt = out_array(fake, "long", n + 1), out_array(fake, "long", 2)
                oo = None if span_cap is None else out_array(fake, "long", span_cap + 1)
                out = None if unit_cap is None else out_array(fake, "char", unit_cap)
                assert call(fake, "gatherMatchesPackedHost", h, data, off, mode, so, oo, out, tt, inputs=(data, off)) == OK, (what, span_cap, unit_cap)
                assert fake.read(tt).tolist() == [len(parts), len(want_text)] and (fake.read(so) == want_span_off).all(), \
                    (what, span_cap, unit_cap, "gather_cases.gather_ref / split_list_ref of oracle.find_all: sizes")
                if unit_cap and unit_cap == len(want_text) and span_cap:
                    assert (fake.read(oo) == want_off).all() and (fake.read(out) == want_text).all(), (what, "gather_cases.gather_ref / split_list_ref of oracle.find_all")


# ---- pattern sets ------------------------------------------------------------------------------------------------------------------
SET_MEMBERS = ["[0-9]+", "(ab|cd)+e?", "x*", "Sherlock|Holmes|Watson"]
SET_UNION = "[0-9]+|(ab|cd)+e?|x+|Sherlock|Holmes|Watson|[α-ω]+"


def make_set(fake):
    members = [shim_pattern(fake, r) for r in SET_MEMBERS]
    out = fake.array("long", [0])
    hs = fake.array("long", [m[0] for m in members])
    assert call(fake, "setCreate", hs, out, inputs=(hs,)) == OK
    return int(fake.read(out)[0]), [m[1] for m in members]


def test_set_natives_against_the_members_oracles(fake):
    """setPackedHost ops 0 / 1 against pattern_set_cases.oracle_masks; setTagMatchesPackedHost against oracle.find_all of the union pattern with
    set_spans_cases.reference_span_masks beside it; setReplaceEachPackedHost against a Python splice by lowest set bit (no bit: kept);
    setMatchesSpansPackedDev (device addresses of torch tensors) against the same span reference."""
    s, oracles = make_set(fake)
    try:
        set_natives(fake, s, oracles)
    finally:
        fake.call("setDestroy", s)


def set_natives(fake, s, oracles):
    import torch
    from pattern_set_cases import oracle_masks
    from set_spans_cases import reference_span_masks, spans_from_lists
    hu, ou = shim_pattern(fake, SET_UNION)
    repls = [J.u16(t) for t in ("<N>", "", "￿X", "detective")]
    repl_all = fake.array("char", np.concatenate(repls))
    repl_off = fake.array("int", np.concatenate([[0], np.cumsum([len(r) for r in repls])]))
    for n, long_row in [(n, False) for n in ROW_COUNTS] + [(64, True)]:
        rows = make_rows(n, 500 + n, long_row=long_row)
        n = len(rows)
        data_np, off_np = pack(rows)
        data, off = fake.array("char", data_np), fake.array("long", off_np)
        want_m, want_c = oracle_masks(oracles, rows, np.uint16) if n else (np.zeros(0, np.uint32), np.zeros(0, np.uint32))
        for op, want in ((0, want_m), (1, want_c)):
            masks = out_array(fake, "int", n)
            assert call(fake, "setPackedHost", s, op, data, off, masks, inputs=(data, off)) == OK, (n, op)
            assert (fake.read(masks).view(np.uint32) == want).all(), ("rows", n, "op", op, "pattern_set_cases.oracle_masks")
        lists = oracle_find_all(ou, rows)
        spans = spans_from_lists(lists)
        want_tags = reference_span_masks(oracles, rows, spans)
        total = len(spans[1])
        for cap in (None, total, total - 1):
            if cap is not None and cap < 0:
                continue
            mo, tt = out_array(fake, "long", n + 1), out_array(fake, "long", 1)
            st, en, mk = (None, None, None) if cap is None else (out_array(fake, "int", cap), out_array(fake, "int", cap), out_array(fake, "int", cap))
            assert call(fake, "setTagMatchesPackedHost", s, hu, data, off, mo, st, en, mk, tt, inputs=(data, off)) == OK, (n, cap)
            assert int(fake.read(tt)[0]) == total and (fake.read(mo) == spans[0]).all(), ("rows", n, cap, "oracle.find_all of the union")
            if cap == total and total:
                assert (fake.read(st) == spans[1]).all() and (fake.read(en) == spans[2]).all(), ("rows", n, "oracle.find_all of the union")
                assert (fake.read(mk).view(np.uint32) == want_tags).all(), ("rows", n, "set_spans_cases.reference_span_masks")
        # replace each match by the replacement of its lowest member; a match no member matches whole is kept
        at, want_rows = 0, []
        for r, m in zip(rows, lists):
            tags = want_tags[at:at + len(m)]
            at += len(m)
            want_rows.append(splice(r, m, [None if t == 0 else repls[int(t & -t).bit_length() - 1] for t in tags.tolist()]))
        want_text, want_off = pack(want_rows)
        for cap in (None, len(want_text), len(want_text) - 1):
            if cap is not None and cap < 0:
                continue
            oo, tt = out_array(fake, "long", n + 1), out_array(fake, "long", 1)
            out = None if cap is None else out_array(fake, "char", cap)
            rc = call(fake, "setReplaceEachPackedHost", s, hu, data, off, repl_all, repl_off, oo, out, tt, inputs=(data, off, repl_all, repl_off))
            assert rc == OK, (n, cap)
            assert int(fake.read(tt)[0]) == len(want_text) and (fake.read(oo) == want_off).all(), ("rows", n, cap, "Python splice by lowest set bit: sizes")
            if cap == len(want_text) and cap:
                assert (fake.read(out) == want_text).all(), ("rows", n, "Python splice by lowest set bit")
        # the device entry: addresses of torch tensors
        if n:
            pad2 = np.concatenate([data_np, np.zeros(data_np.size % 2, np.uint16)])  # (whole 4 bytes)
            d_data = torch.from_numpy(pad2.view(np.int16).copy()).cuda() if pad2.size else torch.zeros(2, dtype=torch.int16, device="cuda")
            d_off, d_so = torch.from_numpy(off_np).cuda(), torch.from_numpy(spans[0]).cuda()
            d_st = torch.from_numpy(np.concatenate([spans[1], [0]]).astype(np.int32)).cuda()
            d_en = torch.from_numpy(np.concatenate([spans[2], [0]]).astype(np.int32)).cuda()
            d_mk = torch.full((total + 1,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
            rc = call(fake, "setMatchesSpansPackedDev", s, d_data.data_ptr(), 2, n, d_off.data_ptr(), d_so.data_ptr(), d_st.data_ptr(), d_en.data_ptr(), d_mk.data_ptr(), 0)
            torch.cuda.synchronize()
            got = d_mk.cpu().numpy()
            assert rc == OK and (got[:total].view(np.uint32) == want_tags).all() and got[total] == 0x5A5A5A5A, ("rows", n, "set_spans_cases.reference_span_masks")


# ---- one Matcher -------------------------------------------------------------------------------------------------------------------
def test_matcher_natives_on_the_recorded_rows(fake):
    """matcherCreate / matcherFind / matcherStart / matcherEnd / matcherFindRange / matcherMatches / matcherContainedIn on 40 rows spread over
    tests/golden/matches.json: find() against the recorded answers, matches() / containedIn() against the oracle."""
    from test_compile_matches_txt import flag_sets
    doc = json.load(open(os.path.join(GOLDEN, "matches.json")))
    picked = doc["rows"][::5]
    assert len(picked) == 40
    for row in picked:
        flags = flag_sets(row)[0]
        h, o = shim_pattern(fake, row["pattern"], flags)
        hay = fake.array("char", J.u16(row["haystack"]))
        out = fake.array("long", [0])
        assert call(fake, "matcherCreate", h, hay, out, inputs=(hay,)) == OK, row
        m = int(fake.read(out)[0])
        r = out_array(fake, "int", 1)
        assert call(fake, "matcherFind", m, r) == OK and bool(fake.read(r)[0]) == row["found"], (row, "recorded answer")
        if row["found"]:
            assert (fake.call("matcherStart", m), fake.call("matcherEnd", m)) == (row["start"], row["end"]), (row, "recorded answer")
        r = out_array(fake, "int", 1)
        assert call(fake, "matcherFindRange", m, 0, len(row["haystack"]), r) == OK and bool(fake.read(r)[0]) == row["found"], (row, "recorded answer")
        if row["found"]:
            assert (fake.call("matcherStart", m), fake.call("matcherEnd", m)) == (row["start"], row["end"]), (row, "recorded answer, find(0, length)")
        r = out_array(fake, "int", 1)
        assert call(fake, "matcherMatches", m, r) == OK and bool(fake.read(r)[0]) == o.matches(row["haystack"]), (row, "oracle.matches")
        r = out_array(fake, "int", 1)
        assert call(fake, "matcherContainedIn", m, r) == OK and bool(fake.read(r)[0]) == o.contained_in(row["haystack"]), (row, "oracle.contained_in")
        fake.call("matcherDestroy", m)
        fake.assert_clean("matcherDestroy")


# ---- fuzz --------------------------------------------------------------------------------------------------------------------------
FUZZ_ALPHABET = [ord(c) for c in "abcxyz019 AB_\n."] + [0xE9, 0x416, 0x4E2D, 0x8000, 0xFFFF]


@pytest.mark.parametrize("seed", range(5))
def test_random_regexes_through_the_shim(fake, seed):
    """Six random_regex draws per seed (the generator of tests/test_compile_vs_python_restatement.py; a draw the compiler refuses is redrawn)
    through packedHost find, findAllPackedHost and replaceAllPackedHost on 257 rows of 0 .. 70 chars, against the oracle."""
    from needle_amd.pattern import PatternException
    from test_compile_matches_txt import oracle_for
    from test_compile_vs_python_restatement import FLAG_SETS, random_regex
    rng, nrng = random.Random(9100 + seed), np.random.default_rng(9100 + seed)
    done = 0
    while done < 6:
        regex, flags = random_regex(rng), rng.choice(FLAG_SETS)
        try:
            o = oracle_for(regex, flags)[0]
        except (PatternException, ValueError):
            continue
        out = fake.array("long", [0])
        assert call(fake, "compile", fake.array("char", J.u16(regex)), flags, out) == OK, (regex, flags, "the Python path compiled it")
        done += 1
        h, what = int(fake.read(out)[0]), (seed, regex, flags)
        rows = [nrng.choice(FUZZ_ALPHABET, int(k)).astype(np.uint16) for k in nrng.integers(0, 71, 257)]
        n = len(rows)
        data_np, off_np = pack(rows)
        data, off = fake.array("char", data_np), fake.array("long", off_np)
        wf, ws, we = oracle_find(o, rows)
        bm, st, en = out_array(fake, "long", (n + 63) // 64), out_array(fake, "int", n), out_array(fake, "int", n)
        assert call(fake, "packedHost", h, 2, data, off, bm, st, en, inputs=(data, off)) == OK, what
        assert (bits(fake.read(bm), n) == wf).all() and (fake.read(st) == ws).all() and (fake.read(en) == we).all(), (what, "oracle.batch_find")
        lists = oracle_find_all(o, rows)
        total = sum(len(m) for m in lists)
        mo, tt, st, en = out_array(fake, "long", n + 1), out_array(fake, "long", 1), out_array(fake, "int", total), out_array(fake, "int", total)
        assert call(fake, "findAllPackedHost", h, data, off, mo, st, en, tt, inputs=(data, off)) == OK, what
        assert int(fake.read(tt)[0]) == total and (fake.read(mo) == np.concatenate([[0], np.cumsum([len(m) for m in lists])])).all(), (what, "oracle.find_all")
        assert list(zip(fake.read(st).tolist(), fake.read(en).tolist())) == [m for per in lists for m in per], (what, "oracle.find_all")
        repl_np = J.u16("中=")
        repl = fake.array("char", repl_np)
        want_text, want_off = pack([splice(r, m, [repl_np] * len(m)) for r, m in zip(rows, lists)])
        oo, tt, text = out_array(fake, "long", n + 1), out_array(fake, "long", 1), out_array(fake, "char", len(want_text))
        assert call(fake, "replaceAllPackedHost", h, data, off, repl, oo, text, tt, inputs=(data, off, repl)) == OK, what
        assert int(fake.read(tt)[0]) == len(want_text) and (fake.read(oo) == want_off).all() and (fake.read(text) == want_text).all(), \
            (what, "oracle.find_all spliced in Python")
        fake.call("destroyPattern", h)
