"""Documents cut into lines on the device (needle_lines_count_packed_dev / needle_lines_fill_packed_dev; lines_packed, lines_of_bytes,
Pattern.grep_lines_bytes / count_lines_bytes): bit-exact against batch_ref (tests/lines_cases.py), no tolerances.  Every run through the
raw entries writes into buffers with 64 sentinel entries in front of and behind the offsets output and the text output (and the tile
counts and the document offsets); they must come back untouched.  T, the units of a tile, is asked of the library."""
import ctypes
import re

import numpy as np
import pytest

from lines_cases import CR, LF, batch_ref, tile_counts_ref
from test_gpu_packed_dev import device_packed
from test_gpu_replace_all import GUARD, check_guarded, guarded

SENT = 0x5A5A5A5A5A5A5A5A  # of the int64 buffers
A, B, SP = ord("a"), ord("b"), ord(" ")


def tile_units(cw):
    from needle_amd import _lib
    T = _lib.lib().needle_lines_tile_units(cw)
    assert T >= 256 and T % 16 == 0
    return T


def dt(cw):
    return np.uint8 if cw == 1 else np.uint16


def guarded64(n):
    """A device int64 tensor of sentinels: GUARD entries, room for n, GUARD more -> (whole, the view behind GUARD)."""
    import torch
    big = torch.full((GUARD + n + GUARD,), SENT, dtype=torch.int64, device="cuda")
    return big, big[GUARD:]


def inner(big, n):
    """The n entries of a guarded64 buffer, after checking the sentinels around them."""
    got = big.cpu().numpy()
    assert (got[:GUARD] == SENT).all() and (got[GUARD + n:] == SENT).all(), "sentinels of an int64 buffer"
    return got[GUARD:GUARD + n]


def check_lines(docs, cw, keep, lead=5, trail=7, junk=None, out_start=0, line_start=0, doc_lines=True, stream=None, what=""):
    """The two raw entries (count, torch cumsum, fill) on the documents against batch_ref: the tile counts, the line offsets, the text, the
    document offsets, and every sentinel."""
    import torch
    from needle_amd import _lib
    L = _lib.lib()
    dtype = dt(cw)
    docs = [np.asarray(d, dtype=dtype) for d in docs]
    want, want_off, want_doc = batch_ref(docs, keep, dtype)
    data, offsets = device_packed(docs, dtype, lead=lead, trail=trail, junk=junk)
    first, units, n, lines = int(offsets[0]), data.numel(), len(docs), want_off.size - 1
    T = tile_units(cw)
    tiles = L.needle_lines_tiles(units, cw)
    assert tiles == -(-units // T)
    v = _lib.PackedView()
    v.data, v.char_width, v.n_rows, v.offsets = data.data_ptr(), cw, n, offsets.data_ptr()
    flags = _lib.LINES_KEEP_ENDS if keep else 0
    s = None if stream is None else stream.cuda_stream
    with torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream()):
        big_tl, tl = guarded64(tiles)
        big_tu, tu = guarded64(tiles)
        assert L.needle_lines_count_packed_dev(ctypes.byref(v), units, flags, tl.data_ptr(), None if keep else tu.data_ptr(), s) == 0, _lib.last_error()
        want_ev, want_kept = tile_counts_ref(docs, first, T, tiles)
        assert (inner(big_tl, tiles) == want_ev).all(), ("tile lines", what)
        assert (inner(big_tu, tiles) == (SENT if keep else want_kept)).all(), ("tile units", what)
        lb = torch.full((tiles + 1,), line_start, dtype=torch.int64, device="cuda")
        ub = torch.full((tiles + 1,), out_start, dtype=torch.int64, device="cuda")
        lb[1:] += torch.cumsum(tl[:tiles], 0)
        if not keep:
            ub[1:] += torch.cumsum(tu[:tiles], 0)
        big_oo, oo = guarded64(line_start + lines + 1)
        big_dl, dl = guarded64(n + 1)
        big, out, sent = guarded(0 if keep else want.size, out_start, dtype)
        assert L.needle_lines_fill_packed_dev(ctypes.byref(v), units, flags, lb.data_ptr(), None if keep else ub.data_ptr(), oo.data_ptr(),
                                              None if keep else out.data_ptr(), dl.data_ptr() if doc_lines else None, s) == 0, _lib.last_error()
        if stream is not None:
            stream.synchronize()
    torch.cuda.synchronize()
    got_oo = inner(big_oo, line_start + lines + 1)
    if units == 0:  # data_units == 0: NEEDLE_OK at once, nothing is written
        assert lines == 0 and (got_oo == SENT).all() and (inner(big_dl, n + 1) == SENT).all(), ("no data", what)
        return data, offsets
    assert (got_oo[:line_start] == SENT).all(), ("offsets in front of line_start", what)
    got_dl = inner(big_dl, n + 1)
    assert (got_dl == (want_doc + line_start if doc_lines else SENT)).all(), ("document line offsets", what, got_dl[:8], want_doc[:8])
    if keep:
        assert (got_oo[line_start:] == want_off + first).all(), ("offsets", what)
        assert (big.cpu().numpy().view(dtype) == sent).all(), ("KEEP writes no text", what)
    else:
        check_guarded(big, sent, want, want_off, oo[line_start:line_start + lines + 1], out_start, dtype, what)
    return data, offsets


def random_doc(rng, k, alphabet=(A, B, SP, LF, CR), p=None):
    return rng.choice(np.array(alphabet), int(k), p=p)


@pytest.mark.gpu
@pytest.mark.parametrize("cw", [1, 2])
@pytest.mark.parametrize("keep", [False, True])
def test_one_document(cw, keep):
    """1. One document of 0, 1, 15, 16, 17, T - 1, T, T + 1 and 3T + 5 units: terminator-rich text, and text with few terminators."""
    T = tile_units(cw)
    rng = np.random.default_rng(10 + cw)
    for k in (0, 1, 15, 16, 17, T - 1, T, T + 1, 3 * T + 5):
        check_lines([random_doc(rng, k)], cw, keep, what=("dense", k))
        check_lines([random_doc(rng, k, p=[0.45, 0.3, 0.22, 0.02, 0.01])], cw, keep, lead=0, trail=0, what=("sparse", k))
    for one in (LF, CR, A):
        check_lines([[one]], cw, keep, lead=0, trail=0, what=("one unit", one))


@pytest.mark.gpu
@pytest.mark.parametrize("cw", [1, 2])
@pytest.mark.parametrize("keep", [False, True])
def test_tile_and_block_edges(cw, keep):
    """2. '\\r' as the last unit in front of an edge with '\\n' first behind it: one line; the same with a document boundary between them:
    two; '\\r' in front of the edge and last in the span, junk '\\n' behind it.  The edge: a tile's, and a 16-byte block's."""
    T = tile_units(cw)
    lead, per = 8, 16 // cw
    for edge in (T, 2 * T, 3 * per, T + per):  # a unit of the data that begins a tile / a block
        total = 2 * T + 8
        body = np.full(total, A, dt(cw))
        r = edge - 1 - lead  # the unit in front of the edge
        body[r], body[r + 1] = CR, LF
        body[r - 3], body[r + 4] = LF, CR
        for docs, what in (([body], "one document"), ([body[:r + 1], body[r + 1:]], "a boundary between"), ([body[:r + 1]], "the span ends"),
                           ([body[:7], body[7:r + 1], [], body[r + 1:]], "an empty document between")):
            data, offsets = check_lines(docs, cw, keep, lead=lead, trail=8, junk=[LF], what=(what, edge))
            host = data.cpu().numpy()
            assert int(offsets[0]) == lead and host[edge - 1] == CR and host[edge] == LF, "the pair lies at the edge"
        tail = np.full(edge - lead, A, dt(cw))  # an unterminated tail in front of the edge, junk '\\n' behind it
        data, offsets = check_lines([tail], cw, keep, lead=lead, trail=8, junk=[LF], what=("a tail ends the span", edge))
        assert int(offsets[-1]) == edge and data.cpu().numpy()[edge] == LF


@pytest.mark.gpu
@pytest.mark.parametrize("cw", [1, 2])
@pytest.mark.parametrize("keep", [False, True])
def test_all_terminators_and_none(cw, keep):
    """3. 2T + 3 units of '\\n', of '\\r', of "\\r\\n" at both parities against the tile edge; no terminator: one line across three tiles."""
    T = tile_units(cw)
    k = 2 * T + 3
    pairs = np.resize(np.array([CR, LF]), k + 1)
    for doc, what in ((np.full(k, LF), "\\n"), (np.full(k, CR), "\\r"), (pairs[:k], "\\r\\n"), (pairs[1:], "\\n\\r"), (np.full(k, A), "none")):
        check_lines([doc], cw, keep, lead=8, trail=1, what=what)
        check_lines([doc[:T + 1], doc[T + 1:]], cw, keep, lead=0, trail=1, what=(what, "two documents"))


@pytest.mark.gpu
@pytest.mark.parametrize("keep", [False, True])
def test_width_2_look_alikes(keep):
    """4. 0x0A0A, 0x010A, 0x0D00, 0x2028, 0x0085 (and 0x0A00, 0x0D0D) are ordinary characters, at tile and block edges and next to real
    terminators: a '\\r' in front of 0x0A0A is a terminator of its own."""
    T = tile_units(2)
    alike = [0x0A0A, 0x010A, 0x0D00, 0x2028, 0x0085, 0x0A00, 0x0D0D]
    body = np.full(2 * T + 40, A, np.uint16)
    for i, edge in enumerate((T, 8, 16, T + 8, 2 * T)):
        for j, x in enumerate(alike):
            body[edge - 4 + (j % 8)] = x  # around the edge, the edge's two units among them
        body[edge - 1], body[edge] = (CR, alike[i]) if i % 2 else (alike[i], LF)
    check_lines([body], 2, keep, lead=0, trail=0, what="look-alikes")
    check_lines([body[:T], body[T:]], 2, keep, lead=0, trail=0, what="look-alikes, two documents")
    check_lines([np.array(alike * 30, np.uint16)], 2, keep, what="look-alikes only")


def mixed_docs(rng, n, cw, max_len=120):
    return [random_doc(rng, k).astype(dt(cw)) for k in rng.integers(0, max_len + 1, n)]


@pytest.mark.gpu
@pytest.mark.parametrize("cw", [1, 2])
@pytest.mark.parametrize("keep", [False, True])
def test_layout(cw, keep):
    """5. offsets[0] of 0, 5 and 133; junk full of '\\n' in front of offsets[0] and behind offsets[n]; data_units well above offsets[n];
    out_start and line_start of 0 and 3."""
    T = tile_units(cw)
    rng = np.random.default_rng(50 + cw)
    docs = mixed_docs(rng, 150, cw)
    for lead in (0, 5, 133):
        for out_start, line_start in ((0, 0), (3, 0), (0, 3), (3, 3)):
            check_lines(docs, cw, keep, lead=lead, trail=7, junk=[LF, CR], out_start=out_start, line_start=line_start,
                        what=("lead", lead, "out_start", out_start, "line_start", line_start))
    check_lines(docs, cw, keep, lead=5, trail=2 * T + 11, junk=[LF], out_start=3, line_start=3, what="data_units well above offsets[n]")
    check_lines(docs[:3], cw, keep, lead=2 * T + 4, trail=T, junk=[LF], what="whole tiles in front of the span")


@pytest.mark.gpu
@pytest.mark.parametrize("cw", [1, 2])
@pytest.mark.parametrize("keep", [False, True])
def test_documents(cw, keep):
    """6. 1, 63, 64, 65 and 700 documents of 0..120 units; empty documents in runs, at the front and at the end; only empty documents; the
    document offsets asked for and not."""
    rng = np.random.default_rng(60 + cw)
    docs = mixed_docs(rng, 700, cw)
    empty = np.zeros(0, dt(cw))
    for n in (1, 63, 64, 65, 700):
        check_lines(docs[:n], cw, keep, what=("documents", n))
        check_lines(docs[:n], cw, keep, doc_lines=False, line_start=3, what=("documents, no document offsets", n))
    runs = [empty] * 5 + docs[:40] + [empty] * 300 + docs[40:45] + [empty] + docs[45:90] + [empty] * 70
    check_lines(runs, cw, keep, lead=5, out_start=3, line_start=3, what="runs of empty documents")
    check_lines(runs, cw, keep, lead=0, trail=0, what="runs of empty documents, offsets[0] = 0")
    for n in (1, 70):
        check_lines([empty] * n, cw, keep, lead=9, trail=9, junk=[LF], line_start=3, what=("only empty documents", n))
        check_lines([empty] * n, cw, keep, lead=0, trail=4, junk=[LF], what=("only empty documents at 0", n))


@pytest.mark.gpu
@pytest.mark.parametrize("part", range(8))
def test_fuzz(part):
    """7. 200 seeded batches (25 a part) over {a, b, \\n, \\r}: up to 3T units, random document cuts, mode and width; a "\\r\\n" straddling
    the first tile edge is planted in every one of them, and is asserted to be there.  No case is skipped."""
    for seed in range(part * 25, part * 25 + 25):
        rng = np.random.default_rng(7000 + seed)
        cw, keep = int(rng.integers(1, 3)), bool(rng.integers(0, 2))
        T = tile_units(cw)
        lead = int(rng.integers(0, 4)) * 4  # (a multiple of 4 units, as the total is: device_packed leaves it as it is)
        total = int(rng.integers((T + 8) // 4, 3 * T // 4 + 1)) * 4
        p = rng.dirichlet([4, 4, 1, 1]) if seed % 3 else [0.25, 0.25, 0.25, 0.25]
        text = random_doc(rng, total, (A, B, LF, CR), p=p).astype(dt(cw))
        text[T - 1 - lead], text[T - lead] = CR, LF
        cuts = np.sort(rng.integers(0, total + 1, int(rng.integers(0, 40))))
        if seed % 4 == 0:
            cuts = np.sort(np.concatenate([cuts, [T - lead]]))  # a document boundary inside the pair
        bounds = [0] + cuts.tolist() + [total]
        docs = [text[a:b] for a, b in zip(bounds, bounds[1:])]
        data, offsets = check_lines(docs, cw, keep, lead=lead, trail=4, junk=[LF], out_start=int(rng.integers(0, 20)), line_start=int(rng.integers(0, 5)),
                                    doc_lines=bool(seed % 5), what=("fuzz", seed))
        host = data.cpu().numpy()
        assert int(offsets[0]) == lead and int(offsets[-1]) > T and host[T - 1] == CR and host[T] == LF, ("the planted pair", seed)


@pytest.mark.gpu
@pytest.mark.parametrize("cw", [1, 2])
def test_keep_invariants_and_python_entry(cw):
    """8. keep_ends: the text is the caller's tensor, the offsets are increasing positions of it and the lines put together are the span.
    And lines_packed in both modes against batch_ref: out / out_start / line_start, no offsets (one document), numpy inputs, no input."""
    import torch
    from needle_amd.pattern import lines_of_bytes, lines_packed
    dtype = dt(cw)
    rng = np.random.default_rng(80 + cw)
    docs = mixed_docs(rng, 200, cw)
    data, offsets = device_packed(docs, dtype, lead=5, trail=7, junk=[LF])
    first, last = int(offsets[0]), int(offsets[-1])
    text, lo, dlo = lines_packed(data, offsets, keep_ends=True)
    want, want_off, want_doc = batch_ref(docs, True, dtype)
    assert text.data_ptr() == data.data_ptr() and text.numel() == data.numel()
    got = lo.cpu().numpy()
    assert got[0] == first and got[-1] == last and (np.diff(got) > 0).all() and (got == want_off + first).all()
    assert (dlo.cpu().numpy() == want_doc).all()
    host = data.cpu().numpy().view(dtype)
    assert (np.concatenate([host[a:b] for a, b in zip(got, got[1:])]) == host[first:last]).all()
    # STRIP through the Python entry, appending behind 3 units and 2 lines
    want, want_off, want_doc = batch_ref(docs, False, dtype)
    big, out, sent = guarded(want.size, 3, dtype)
    text, lo, dlo = lines_packed(data, offsets, out=out, out_start=3, line_start=2)
    torch.cuda.synchronize()
    assert text.data_ptr() == out.data_ptr() and lo.numel() == want_off.size + 2 and (lo[:2].cpu().numpy() == 3).all()
    check_guarded(big, sent, want, want_off, lo[2:], 3, dtype, "lines_packed, out")
    assert (dlo.cpu().numpy() == want_doc + 2).all()
    # one document: the whole tensor; numpy in, numpy out
    whole = np.concatenate(docs)
    for keep in (False, True):
        want, want_off, want_doc = batch_ref([whole], keep, dtype)
        t, lo, dlo = lines_packed(whole, keep_ends=keep)
        assert isinstance(t, np.ndarray) and t.dtype == dtype and (t[:want.size] == want).all() and (lo == want_off).all() and (dlo == want_doc).all()
        pad = np.concatenate([whole, np.zeros((-whole.size) % (4 // cw), dtype)])
        t, lo, dlo = lines_packed(torch.from_numpy(pad.view(np.uint8 if cw == 1 else np.int16)).to("cuda")[:whole.size], keep_ends=keep)
        assert (t.cpu().numpy().view(dtype)[:want.size] == want).all() and (lo.cpu().numpy() == want_off).all()
        t, lo, dlo = lines_packed(np.zeros(0, dtype), keep_ends=keep)
        assert t.size == 0 and lo.tolist() == [0] and dlo.tolist() == [0, 0]
    if cw == 1:
        b = whole.tobytes()
        assert lines_of_bytes(b) == b.splitlines() and lines_of_bytes(b, keep_ends=True) == b.splitlines(keepends=True)
        assert lines_of_bytes(b"") == [] and lines_of_bytes(b"\n") == [b""] and lines_of_bytes(b"a") == [b"a"]


@pytest.mark.gpu
@pytest.mark.parametrize("cw", [1, 2])
@pytest.mark.parametrize("keep", [False, True])
def test_wrong_bases(cw, keep):
    """9. Bases that are not the prefix sums of the counts -- all equal; half the counts; shifted by 5 -- give unspecified lines and never a
    write outside entries [line_base[0], line_base[tiles]] of the offsets and units [unit_base[0], unit_base[tiles]) of the text: only
    the sentinels are checked.  The bases stay inside the buffers."""
    import torch
    from needle_amd import _lib
    L = _lib.lib()
    dtype = dt(cw)
    T = tile_units(cw)
    rng = np.random.default_rng(90 + cw)
    docs = mixed_docs(rng, 500, cw)
    want, want_off, _ = batch_ref(docs, keep, dtype)
    data, offsets = device_packed(docs, dtype, lead=5, trail=7)
    units, lines = data.numel(), want_off.size - 1
    tiles = L.needle_lines_tiles(units, cw)
    assert tiles >= 3
    ev, kept = tile_counts_ref(docs, int(offsets[0]), T, tiles)
    v = _lib.PackedView()
    v.data, v.char_width, v.n_rows, v.offsets = data.data_ptr(), cw, len(docs), offsets.data_ptr()
    base = lambda c: np.concatenate([[0], np.cumsum(c)]).astype(np.int64)
    for name, lb, ub in (("all equal", np.zeros(tiles + 1, np.int64), np.zeros(tiles + 1, np.int64)), ("half", base(ev // 2), base(kept // 2)),
                         ("lines right, units half", base(ev), base(kept // 2)), ("shifted", base(ev) + 5, base(kept) + 5)):
        for start in (0, 3):
            lb2, ub2 = lb + start, ub + start
            big_oo, oo = guarded64(lines + 9)
            big, out, sent = guarded(want.size + 8, 0, dtype)
            d_lb, d_ub = torch.from_numpy(lb2).to("cuda"), torch.from_numpy(ub2).to("cuda")
            assert L.needle_lines_fill_packed_dev(ctypes.byref(v), units, 1 if keep else 0, d_lb.data_ptr(), None if keep else d_ub.data_ptr(), oo.data_ptr(),
                                                  None if keep else out.data_ptr(), None, None) == 0, _lib.last_error()
            torch.cuda.synchronize()
            got = big_oo.cpu().numpy()
            assert (got[:GUARD + lb2[0]] == SENT).all() and (got[GUARD + lb2[-1] + 1:] == SENT).all(), (name, start, "offsets")
            got = big.cpu().numpy().view(dtype)
            a, b = (GUARD, GUARD) if keep else (GUARD + int(ub2[0]), GUARD + int(ub2[-1]))
            assert (got[:a] == sent).all() and (got[b:] == sent).all(), (name, start, "text")


@pytest.mark.gpu
@pytest.mark.parametrize("keep", [False, True])
def test_callers_stream(keep):
    """10. Both entries on a stream of the caller's, and lines_packed with stream=."""
    import torch
    from needle_amd.pattern import lines_packed
    rng = np.random.default_rng(100)
    docs = mixed_docs(rng, 300, 1)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    data, offsets = check_lines(docs, 1, keep, stream=side, out_start=3, what="side stream")
    want, want_off, want_doc = batch_ref(docs, keep, np.uint8)
    text, lo, dlo = lines_packed(data, offsets, keep_ends=keep, stream=side.cuda_stream)
    side.synchronize()
    assert (lo.cpu().numpy() == want_off + (int(offsets[0]) if keep else 0)).all() and (dlo.cpu().numpy() == want_doc).all()
    assert keep or (text.cpu().numpy() == want).all()


def make_log(seed=11, n_lines=3000):
    """A UTF-8 "log": lines with multi-byte text, "ERROR <number>" in some, mixed '\\n' / "\\r\\n" ends, a few ill-formed bytes."""
    import random
    rng = random.Random(seed)
    words = ["GET /index", "ERROR 404", "ERROR", "error 7", "Zürich", "中文日志", "ERROR 5 😀", "naïve café", "WARN", "ERROR x1", "x" * 150, ""]
    out = bytearray()
    for i in range(n_lines):
        line = bytearray(" ".join(rng.choice(words) for _ in range(rng.randint(0, 6))).encode("utf-8"))
        if i % 97 == 0 and line:
            line[rng.randrange(len(line))] = rng.choice([0xFF, 0xC3, 0xE4, 0x80])
        out += line + (b"\r\n" if rng.random() < 0.4 else b"\n")
    return bytes(out) + b"ERROR 99 unterminated"


@pytest.mark.gpu
def test_chain():
    """11. A file goes upload -> lines -> contained_in_utf8_packed -> select_rows_packed: grep_lines_bytes and count_lines_bytes, three
    times each, against re.search on the decoded lines of bytes.splitlines; the same file as two documents through lines_packed and the
    same chain, the scan called four times back to back."""
    import torch
    from needle_amd.pattern import DFACompiler, Pattern, lines_packed, unpack_bitmap
    buf = make_log()
    p = DFACompiler.compile("ERROR [0-9]+")
    rx = re.compile("ERROR [0-9]+")
    all_lines = buf.splitlines()
    want = [l for l in all_lines if rx.search(l.decode("utf-8", "replace"))]
    assert len(all_lines) == 3001 and 300 < len(want) < 2700 and buf.count(b"\r\n") > 500 and any(b"\xff" in l for l in all_lines)
    for _ in range(3):  # (a pattern's first call uploads its program and waits for the device; the later ones do not)
        assert p.grep_lines_bytes(buf) == want
        assert p.count_lines_bytes(buf) == len(want)
    assert p.grep_lines_bytes(b"") == [] and p.count_lines_bytes(b"") == 0 and p.grep_lines_bytes(b"\n\n") == []
    # two documents: the cut falls inside a line, which becomes two
    cut = len(buf) // 2
    assert buf[cut - 1:cut] not in (b"\n", b"\r")
    a = np.frombuffer(buf, np.uint8)
    d = torch.from_numpy(np.concatenate([a, np.zeros(4 + (-a.size) % 4, np.uint8)])).to("cuda")
    off = torch.tensor([0, cut, len(buf)], dtype=torch.int64, device="cuda")
    text, lo, dlo = lines_packed(d, off)
    halves = buf[:cut].splitlines() + buf[cut:].splitlines()
    assert dlo.tolist() == [0, len(buf[:cut].splitlines()), len(halves)] and lo.numel() == len(halves) + 1
    want_hit = [bool(rx.search(l.decode("utf-8", "replace"))) for l in halves]
    calls = [p.contained_in_utf8_packed(text, lo) for _ in range(4)]  # back to back: nothing waits for the device between them
    for bits in calls:
        assert unpack_bitmap(bits, len(halves)).tolist() == want_hit
    hit = unpack_bitmap(bits, len(halves))
    got, goff = Pattern.select_rows_packed(text, lo, bits)
    got, goff = got.cpu().numpy(), goff.cpu().numpy()
    assert [got[goff[i]:goff[i + 1]].tobytes() for i in range(goff.size - 1)] == [l for l, h in zip(halves, hit) if h]
