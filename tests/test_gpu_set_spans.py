"""Tags for a match list on the GPU (needle_set_matches_spans_packed_dev, the kernel of needle_set_spans.h; needle_set_tag_matches_packed_host):
whole rows as spans against the row masks, the union pattern's match list against the oracle per member, arbitrary and malformed
spans, the shapes where the lane <-> span mapping can go wrong, several groups, the host entry in several chunks, and 20 000 rows of
the 32-keyword set against a plain text comparison."""
import numpy as np
import pytest

from pattern_set_cases import KW32, SETS, assert_plan, compile_set, oracle_masks, split_case, units
from set_spans_cases import random_spans, reference_span_masks, spans_from_lists, union_spans
from test_gpu_pattern_set import JUNK, run_child

pytestmark = pytest.mark.gpu

SENTINEL = 0x5A5A5A5A
# (count260 / count260ci: the matches products have more than 255 states -- set_spans_kernel with 16-bit table elements, both widths)
NAMES = ["nullable4", "logs8", "u16b", "count260", "count260@16", "count260ci@8", "count260ci"]


@pytest.fixture(scope="module", autouse=True)
def built():
    from needle_amd import build
    build.build()
    from oracle import walker
    walker.build()


_cache = {}


def case(name):
    """(set, per-member oracles, dtype, rows, device data, device offsets) of a set: the batch recipe with offsets[0] > 0 and text that
    matches the members around the rows -- computed once per set."""
    if name not in _cache:
        from test_gpu_packed_dev import device_packed
        set_name, dtype = split_case(name)
        ps, oracles, dtype = compile_set(set_name, dtype)
        if set_name.startswith("count260"):  # the plan about to run: 16-bit table elements
            assert assert_plan(set_name, ps, "matches", np.dtype(dtype).itemsize)["kernel_mode"] == 2
        rows = union_spans(name)[0]
        data, offsets = device_packed(rows, dtype, lead=5, trail=7, junk=units(JUNK[set_name], dtype))
        assert int(offsets[0]) > 0
        _cache[name] = (ps, oracles, dtype, rows, data, offsets)
    return _cache[name]


def device_span_masks(ps, data, offsets, spans, front=0, behind=0, fill=SENTINEL):
    """The entry on a host span list -> uint32[M + behind]: the masks tensor is pre-filled with `fill`, `behind` more entries follow
    the list's (the `front` ones are the list's own first span_offsets[0] entries)."""
    import torch
    off, start, end = spans
    assert int(off[0]) == front
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to("cuda")
    out = torch.full((len(start) + behind,), fill, dtype=torch.int32, device="cuda")
    got = ps.matches_spans_packed(data, offsets, dev(off), dev(start), dev(end), out=out)
    torch.cuda.synchronize()
    assert got is out
    return out.cpu().numpy().view(np.uint32)


def check(got, want, spans, k, what, behind=0):
    off = spans[0]
    lo, hi = int(off[0]), int(off[-1])
    assert (got[:lo] == SENTINEL).all() and (got[hi:] == SENTINEL).all() and got.size == hi + behind, (what, "entries that are nobody's were written")
    bad = lo + np.nonzero(got[lo:hi] != want[lo:hi])[0]
    assert bad.size == 0, (what, bad[:10], got[bad[:5]], want[bad[:5]], spans[1][bad[:5]], spans[2][bad[:5]])
    assert not (got[lo:hi] >> np.uint32(k)).any(), (what, "bits at or above n_patterns")


@pytest.mark.parametrize("name", NAMES)
def test_whole_rows_as_spans_equal_the_row_masks(name):
    """One span [0, len) per row: the masks of matches_packed on the same batch and the oracle's -- the 6000- and 9000-char rows are
    spans over many blocks, the 64 empty rows empty spans (the members whose root accepts)."""
    import torch
    ps, oracles, dtype, rows, data, offsets = case(name)
    spans = spans_from_lists([[(0, len(r))] for r in rows])
    got = device_span_masks(ps, data, offsets, spans)
    row_masks = ps.matches_packed(data, offsets)
    torch.cuda.synchronize()
    want = oracle_masks(oracles, rows, dtype)[0]
    assert (row_masks.cpu().numpy().view(np.uint32) == want).all()
    check(got, want, spans, len(oracles), name)
    if name == "nullable4":
        assert all(got[r] & 1 for r in range(128, 192)), "an empty span: the root-accepting member's bit"


@pytest.mark.parametrize("name", NAMES)
def test_union_spans_are_tagged_with_their_members(name):
    """tag_matches_packed(union_pattern()): the oracle's match list of the union, and per span the members whose oracle matches it."""
    import torch
    ps, oracles, dtype, rows, data, offsets = case(name)
    _, want_spans = union_spans(name)
    off, st, en, masks = ps.tag_matches_packed(ps.union_pattern(), data, offsets)
    torch.cuda.synchronize()
    assert masks.is_cuda and masks.dtype == torch.int32 and masks.numel() == st.numel()
    assert (off.cpu().numpy() == want_spans[0]).all() and (st.cpu().numpy() == want_spans[1]).all() and (en.cpu().numpy() == want_spans[2]).all()
    got = masks.cpu().numpy().view(np.uint32)
    want = reference_span_masks(oracles, rows, want_spans)
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, (name, bad[:10], got[bad[:5]], want[bad[:5]])
    assert (want != 0).all() and (ps.first_member(masks) >= 0).all()  # (nullable4's empty spans: the nullable member, bit 0)


@pytest.mark.parametrize("name", NAMES)
def test_arbitrary_and_malformed_spans(name):
    """random_spans -- every length class, every alignment, unordered and overlapping, negative s / e > len / e < s -- against the
    oracle on the clamped spans; span_offsets[0] = 3, sentinels in front of and behind the owned entries."""
    ps, oracles, dtype, rows, data, offsets = case(name)
    rng = np.random.default_rng(5)
    spans = random_spans(rows, rng, abs0=int(offsets[0]), cw=np.dtype(dtype).itemsize, lead=3)
    assert int(spans[0][0]) == 3
    got = device_span_masks(ps, data, offsets, spans, front=3, behind=5)
    want = reference_span_masks(oracles, rows, spans)
    assert (want < (1 << len(oracles))).all()  # (no mask is the sentinel: an owned entry left alone would differ from its answer)
    check(got, want, spans, len(oracles), name, behind=5)


def test_lane_to_span_shapes():
    """One row with 300 spans between rows with none (rounds of 64 and a partial last one); a 64-row group without spans; batches of
    1 and 65 rows; a batch without any span and start / end NULL."""
    import torch
    from test_gpu_packed_dev import device_packed
    ps, oracles, dtype, rows, data, offsets = case("logs8")
    rng = np.random.default_rng(6)
    k = len(oracles)
    # 300 spans in row 70 (6000 chars), none in its group's other rows; rows 128 .. 191 (a whole group) have none; a few behind them
    per_row = [[] for _ in rows]
    n70 = len(rows[70])
    for _ in range(300):
        s = int(rng.integers(0, n70 - 40))
        per_row[70].append((s, s + int(rng.integers(0, 40))))
    for r in (0, 63, 192, 256):
        per_row[r] = [(0, len(rows[r])), (1, 3)]
    spans = spans_from_lists(per_row)
    check(device_span_masks(ps, data, offsets, spans), reference_span_masks(oracles, rows, spans), spans, k, "300 spans in one row")
    for n in (1, 65):
        some = [rows[(7 * i) % len(rows)] for i in range(n)]  # (the planted pieces among them: whole-row matches)
        d, o = device_packed(some, dtype, lead=5, trail=7, junk=units(JUNK["logs8"], dtype))
        spans = spans_from_lists([[(0, len(r)), (0, 1)] for r in some])
        want = reference_span_masks(oracles, some, spans)
        assert want.any()
        check(device_span_masks(ps, d, o, spans), want, spans, k, "n_rows %d" % n)
    # no spans at all: the C entry with start / end NULL launches and writes nothing
    import ctypes
    from needle_amd import _lib
    no_spans = torch.zeros(len(rows) + 1, dtype=torch.int64, device="cuda")
    out = torch.full((4,), SENTINEL, dtype=torch.int32, device="cuda")
    v = _lib.PackedView()
    v.data, v.char_width, v.n_rows, v.offsets = data.data_ptr(), data.element_size(), len(rows), offsets.data_ptr()
    s = torch.cuda.current_stream().cuda_stream
    assert _lib.lib().needle_set_matches_spans_packed_dev(ps._h, ctypes.byref(v), no_spans.data_ptr(), None, None, out.data_ptr(), s) == 0
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == SENTINEL).all()


def test_a_batch_without_any_match_gives_empty_results():
    """tag_matches_packed and matches_spans_packed (without and with out=) on a batch in which the pattern finds nothing: four empty,
    well-typed results, a caller's tensor untouched."""
    import torch
    from test_gpu_packed_dev import device_packed
    ps, _, dtype = compile_set("kw32")
    rows = [units("zzzz qqqq", dtype), np.zeros(0, dtype), units("x", dtype)] * 30  # (no keyword: 90 rows, two groups)
    data, offsets = device_packed(rows, dtype, lead=5, trail=7)
    off, st, en, masks = ps.tag_matches_packed(ps.union_pattern(), data, offsets)
    torch.cuda.synchronize()
    assert off.dtype == torch.int64 and off.numel() == len(rows) + 1 and not off.cpu().numpy().any()
    for t in (st, en, masks):
        assert t.is_cuda and t.dtype == torch.int32 and t.numel() == 0
    got = ps.matches_spans_packed(data, offsets, off, st, en)
    assert got.is_cuda and got.dtype == torch.int32 and got.numel() == 0
    out = torch.full((4,), SENTINEL, dtype=torch.int32, device="cuda")
    assert ps.matches_spans_packed(data, offsets, off, st, en, out=out) is out
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == SENTINEL).all()
    assert ps.first_member(masks).size == 0


def test_several_groups_store_then_or():
    """The logs8 union spans with the table budget lowered so that the set is cut into groups: the same masks, into a tensor pre-filled
    with garbage (group 0 stores, later groups read-modify-write)."""
    run_child("import numpy as np\n"
              "from oracle import walker; walker.build()\n"
              "from pattern_set_cases import compile_set, units\n"
              "from set_spans_cases import reference_span_masks, union_spans\n"
              "from test_gpu_packed_dev import device_packed\n"
              "from test_gpu_set_spans import check, device_span_masks\n"
              "ps, oracles, dtype = compile_set('logs8')\n"
              "assert ps.info('matches', 1)['n_groups'] >= 2, ps.info('matches', 1)\n"
              "rows, spans = union_spans('logs8')\n"
              "data, offsets = device_packed(rows, dtype, lead=5, trail=7, junk=units('42 ERROR a-c Holmes ', dtype))\n"
              "got = device_span_masks(ps, data, offsets, spans, fill=-1)\n"
              "want = reference_span_masks(oracles, rows, spans)\n"
              "assert want.all() and (got == want).all(), np.nonzero(got != want)[0][:10]\n"
              "print('CHILD OK')\n", {"NEEDLE_MAX_PROG_LDS": "4096"})


def test_host_entry_in_several_chunks():
    """find_all_tagged_strings on 300 strings with NEEDLE_HOST_CHUNK_BYTES small enough for several chunks and NEEDLE_HOST_RESULT_BYTES
    for several sub-ranges a chunk; capacity 0 sizes without writing; a capacity below the total delivers the leading chunks' rows --
    all of them, worked out from the chunk rule (test_host_plan.packed_chunks) -- nothing behind them, and reports the exact total."""
    run_child("import ctypes\n"
              "import numpy as np\n"
              "from oracle import walker; walker.build()\n"
              "from needle_amd import _lib\n"
              "from needle_amd.pattern import pack_strings\n"
              "from pattern_set_cases import compile_set, gpu_batch, units\n"
              "from set_spans_cases import reference_span_masks, spans_from_lists, union_regex\n"
              "from test_compile_matches_txt import oracle_for\n"
              "from test_host_plan import packed_chunks\n"
              "for name in ('u16b', 'logs8'):\n"
              "    ps, oracles, dtype = compile_set(name)\n"
              "    rows = [r for r in gpu_batch(name) if r.size < 300] + gpu_batch(name, seed=9)[:60]\n"
              "    rows = [r.astype(np.uint16) for r in rows[:300]]\n"
              "    assert len(rows) == 300 and sum(r.size for r in rows) * 2 > 3 * 4096\n"
              "    strings = [''.join(chr(int(c)) for c in r) for r in rows]\n"
              "    uo = oracle_for(union_regex(name), 0)[0]\n"
              "    per_row = [uo.find_all(r) for r in rows]\n"
              "    spans = spans_from_lists(per_row)\n"
              "    want = reference_span_masks(oracles, rows, spans)\n"
              "    u = ps.union_pattern()\n"
              "    got = ps.find_all_tagged_strings(u, strings)\n"
              "    assert len(got) == 300 and sum(len(g) for g in got) == want.size > 100\n"
              "    for r in range(300):\n"
              "        a, b = int(spans[0][r]), int(spans[0][r + 1])\n"
              "        assert got[r] == [(s, e, int(m)) for (s, e), m in zip(per_row[r], want[a:b])], (name, r)\n"
              "    data, offsets = pack_strings(strings)\n"
              "    v = _lib.PackedView()\n"
              "    v.data, v.char_width, v.n_rows, v.offsets = data.ctypes.data, 2, 300, offsets.ctypes.data\n"
              "    fn = _lib.lib().needle_set_tag_matches_packed_host\n"
              "    out, total = np.full(301, 9, np.uint64), ctypes.c_uint64(0)\n"
              "    assert fn(ps._h, u._h, ctypes.byref(v), out.ctypes.data, None, None, None, 0, ctypes.byref(total)) == 0\n"
              "    assert total.value == want.size and (out.astype(np.int64) == spans[0]).all()\n"
              "    cap = int(spans[0][150])\n"
              "    assert 0 < cap < want.size\n"
              "    st, en, mk = np.full(cap + 4, -7, np.int32), np.full(cap + 4, -7, np.int32), np.full(cap + 4, 0x5A5A5A5A, np.uint32)\n"
              "    assert fn(ps._h, u._h, ctypes.byref(v), out.ctypes.data, st.ctypes.data, en.ctypes.data, mk.ctypes.data, cap, ctypes.byref(total)) == 0\n"
              "    assert total.value == want.size and (out.astype(np.int64) == spans[0]).all()\n"
              "    assert (st[cap:] == -7).all() and (en[cap:] == -7).all() and (mk[cap:] == 0x5A5A5A5A).all()\n"
              "    # delivered: every row chunk (12 bytes a row beside the text, 4096 bytes a chunk) whose matches end within the capacity\n"
              "    chunks = packed_chunks([int(x) for x in offsets], 2, 12, 1, 4096)\n"
              "    fit = [r1 for _, r1 in chunks if int(spans[0][r1]) <= cap]\n"
              "    assert 2 <= len(fit) < len(chunks)\n"
              "    d = int(spans[0][fit[-1]])\n"
              "    assert 0 < d <= cap\n"
              "    # (NEEDLE_HOST_RESULT_BYTES: 3 matches a sub-range -- some delivered chunk is filled, tagged and downloaded in several)\n"
              "    assert any(int(spans[0][r1] - spans[0][r0]) > 6 for r0, r1 in chunks if r1 <= fit[-1])\n"
              "    assert (st[:d] == spans[1][:d]).all() and (en[:d] == spans[2][:d]).all() and (mk[:d] == want[:d]).all()\n"
              "    assert (st[d:] == -7).all() and (en[d:] == -7).all() and (mk[d:] == 0x5A5A5A5A).all()\n"
              "print('CHILD OK')\n", {"NEEDLE_HOST_CHUNK_BYTES": "4096", "NEEDLE_HOST_RESULT_BYTES": "36"})


def test_kw32_spans_equal_the_keyword_under_them():
    """20 000 rows of the kw32 recipe: bit i of a span's mask is set exactly when the span's text IS keyword i -- a numpy comparison,
    no oracle; the batch has rows with three and more spans."""
    import torch
    from test_gpu_packed_dev import device_packed
    ps, _, dtype = compile_set("kw32")
    rng = np.random.default_rng(12)
    n = 20000
    alpha = units(SETS["kw32"][2], dtype)
    lens = rng.integers(0, 97, n)
    rows = []
    for i in range(n):
        row = rng.choice(alpha, int(lens[i])).astype(dtype)
        for _ in range(int(rng.integers(0, 5))):
            w = units(KW32[int(rng.integers(32))], dtype)
            if w.size <= row.size:
                at = int(rng.integers(0, row.size - w.size + 1))
                row[at:at + w.size] = w
        rows.append(row)
    data, offsets = device_packed(rows, dtype, lead=5, trail=0)
    off, st, en, masks = ps.tag_matches_packed(ps.union_pattern(), data, offsets)
    torch.cuda.synchronize()
    off, st, en, got = off.cpu().numpy(), st.cpu().numpy(), en.cpu().numpy(), masks.cpu().numpy().view(np.uint32)
    per_row = np.diff(off)
    assert got.size == off[-1] > n // 2 and int((per_row >= 3).sum()) >= 3, np.bincount(per_row)[:8]
    host = data.cpu().numpy()
    base = np.repeat(offsets.cpu().numpy()[:-1], per_row)  # every span's row start
    length = en - st
    want = np.zeros(got.size, np.uint32)
    for i, w in enumerate(KW32):
        wu = units(w, dtype)
        idx = np.nonzero(length == wu.size)[0]
        text = host[(base[idx] + st[idx])[:, None] + np.arange(wu.size)[None, :]]
        want[idx[(text == wu[None, :]).all(axis=1)]] |= np.uint32(1) << np.uint32(i)
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, (bad[:10], got[bad[:5]], want[bad[:5]])
    assert (want != 0).all() and all(int(((want >> np.uint32(i)) & 1).sum()) >= 3 for i in range(32))
    assert (ps.first_member(masks) >= 0).all()
