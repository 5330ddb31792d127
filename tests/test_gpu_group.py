"""Distinct spans and their counts on the GPU (needle_group_spans_packed_dev, the kernels of needle_group.hip) against the model of
group_cases.py: every alignment against every other, the lengths around the 16-byte blocks, texts that differ in one unit, the shapes
where the lane <-> span mapping can go wrong, the comparison path through low hash_bits, contention, long spans, malformed and absent
spans, overflow, determinism, the Python chain end to end, and a fuzz.  Outputs are pre-filled with sentinels, junk surrounds the text
and offsets[0] > 0."""
import collections
import ctypes

import numpy as np
import pytest

from group_cases import NONE, distinct_ref, group_ref
from set_spans_cases import random_spans, spans_from_lists

pytestmark = pytest.mark.gpu

S_FIRST, S_COUNT, S_STATUS = 0x5A5A5A5A5A5A5A5A, 0x5A5A5A5A, 0x5A5A5A5A
DTYPES = [np.uint8, np.uint16]
LENGTHS = [0, 1, 15, 16, 17, 31, 32, 33, 47, 48, 49]


@pytest.fixture(scope="module", autouse=True)
def built():
    from needle_amd import build
    build.build()


def device_rows(rows, dtype, seed=1):
    """device_packed with `lead` / `trail` junk of the rows' own alphabet (never zeros: a unit read from outside a span would show)."""
    from test_gpu_packed_dev import device_packed
    junk = np.random.default_rng(seed).integers(1, 200, 37).astype(dtype)
    data, offsets = device_packed(rows, dtype, lead=5, trail=7, junk=junk)
    assert int(offsets[0]) > 0
    return data, offsets


def run_group(data, offsets, spans, hash_bits=64, behind=0, max_spans=None, work_bytes=None, stream=None, n_rows=None, null_lists=False):
    """The C entry on a host span list -> (rc, status, first uint64[M + behind], count uint32[M + behind]); the outputs and the status
    are pre-filled with sentinels, `behind` more entries follow the list's."""
    import torch
    from needle_amd import _lib
    L = _lib.lib()
    off, start, end = spans
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to("cuda")
    m = len(start)
    d_off, d_st, d_en = dev(off), dev(np.append(start, 0).astype(np.int32)), dev(np.append(end, 0).astype(np.int32))  # (never empty)
    first = torch.full((m + behind + 1,), S_FIRST, dtype=torch.int64, device="cuda")
    count = torch.full((m + behind + 1,), S_COUNT, dtype=torch.int32, device="cuda")
    status = torch.full((1,), S_STATUS, dtype=torch.int32, device="cuda")
    max_spans = m if max_spans is None else max_spans
    work_bytes = int(L.needle_group_spans_work_bytes(max_spans)) if work_bytes is None else work_bytes
    work = torch.full(((work_bytes + 7) // 8,), -1, dtype=torch.int64, device="cuda")  # (garbage: the entry clears what needs clearing)
    v = _lib.PackedView()
    v.data, v.char_width, v.offsets = data.data_ptr(), data.element_size(), offsets.data_ptr()
    v.n_rows = offsets.numel() - 1 if n_rows is None else n_rows
    one = torch.cuda.current_stream() if stream is None else stream
    with torch.cuda.stream(one):
        rc = L.needle_group_spans_packed_dev(ctypes.byref(v), d_off.data_ptr(), None if null_lists else d_st.data_ptr(),
                                             None if null_lists else d_en.data_ptr(), max_spans, hash_bits, work.data_ptr(), work_bytes,
                                             first.data_ptr(), count.data_ptr(), status.data_ptr(), one.cuda_stream)
    one.synchronize()
    f, c = first.cpu().numpy().view(np.uint64), count.cpu().numpy().view(np.uint32)
    assert f[-1] == S_FIRST and c[-1] == S_COUNT
    return rc, int(status.cpu().numpy().view(np.uint32)[0]), f[:-1], c[:-1]


def check(rows, data, offsets, spans, what, hash_bits=64, behind=0, **kw):
    """Run, compare with the model inside [M0, M1), demand the sentinels outside -> (first, count)."""
    rc, status, first, count = run_group(data, offsets, spans, hash_bits=hash_bits, behind=behind, **kw)
    assert (rc, status) == (0, 0), (what, rc, status)
    want_f, want_c = group_ref(rows, spans, S_FIRST, S_COUNT)
    want_f, want_c = np.concatenate([want_f, np.full(behind, S_FIRST, np.uint64)]), np.concatenate([want_c, np.full(behind, S_COUNT, np.uint32)])
    bad = np.nonzero((first != want_f) | (count != want_c))[0]
    assert bad.size == 0, (what, hash_bits, bad[:10], first[bad[:5]], want_f[bad[:5]], count[bad[:5]], want_c[bad[:5]])
    return first, count


def phased_rows(dtype, rng):
    """Rows of whole 16 bytes that hold one text each behind a pad of 0 .. 15 bytes: per length of LENGTHS a base text, the text with
    its first unit changed, with its last unit changed, its prefix and the text plus a trailing unit 0 -- every variant at every byte
    phase (all rows begin at the same phase, the pad runs through all of them) -> (rows, span list, distinct texts)."""
    cw = np.dtype(dtype).itemsize
    rows, per_row, texts = [], [], set()
    for L in LENGTHS:
        base = rng.integers(1, 250, L).astype(dtype)
        variants = [base, np.append(base, 0).astype(dtype)]
        if L:
            variants += [base[:-1]]
            for at in (0, L - 1):
                v = base.copy()
                v[at] ^= 0x40
                variants.append(v)
        for v in variants:
            texts.add(v.tobytes())
            for pad in range(0, 16, cw):
                p = pad // cw
                tail = (-(p + v.size)) % (16 // cw) + (16 // cw) * int(rng.integers(0, 2))
                rows.append(np.concatenate([rng.integers(1, 250, p).astype(dtype), v, rng.integers(1, 250, tail).astype(dtype)]))
                per_row.append([(p, p + v.size)])
    return rows, per_row, texts


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("hash_bits", [64, 0])
def test_alignments_and_lengths(dtype, hash_bits):
    """The same texts at all 16 byte phases against each other group; texts that differ in the first unit only, in the last unit only,
    by a missing last unit or by a trailing unit 0 do not; all empty spans are one group."""
    rng = np.random.default_rng(3)
    cw = np.dtype(dtype).itemsize
    rows, per_row, texts = phased_rows(dtype, rng)
    order = rng.permutation(len(rows))  # (equal texts far apart: in different 64-row groups, waves and workgroups)
    rows, per_row = [rows[i] for i in order], [per_row[i] for i in order]
    spans = spans_from_lists(per_row, lead=3)
    data, offsets = device_rows(rows, dtype)
    # every text was really seen at every phase of its first absolute byte
    seen = collections.defaultdict(set)
    host_off = offsets.cpu().numpy()
    for r, row in enumerate(rows):
        s, e = per_row[r][0]
        seen[row[s:e].tobytes()].add(int((host_off[r] + s) * cw) % 16)
    assert set(seen) == texts and all(len(v) == 16 // cw for t, v in seen.items() if t), {t: sorted(v) for t, v in seen.items() if len(v) != 16 // cw}
    first, count = check(rows, data, offsets, spans, "phases", hash_bits=hash_bits, behind=5)
    lo, hi = int(spans[0][0]), int(spans[0][-1])
    assert int((first[lo:hi] == np.arange(lo, hi)).sum()) == len(texts)
    assert set(count[lo:hi].tolist()) == {16 // cw, 2 * (16 // cw)}  # (the empty text: the base of length 0 and the prefix of length 1)


def small_rows(n, dtype, rng, alphabet=(97, 98), max_len=12):
    return [rng.choice(np.array(alphabet), int(rng.integers(0, max_len + 1))).astype(dtype) for _ in range(n)]


def short_spans(rows, rng, per_row=2, max_len=4):
    out = []
    for row in rows:
        mine = []
        for _ in range(per_row):
            s = int(rng.integers(0, len(row) + 1))
            mine.append((s, s + int(rng.integers(0, max_len + 1))))
        out.append(mine)
    return out


@pytest.mark.parametrize("dtype", DTYPES)
def test_row_counts_and_lane_to_span_shapes(dtype):
    """1, 63, 64, 65, 129 rows; a 64-row group without spans between groups with spans; a 65-row batch whose only spans are in the last
    row; one row with 1000 spans; span_offsets[0] = 3 and five foreign entries behind the list, all left as they were."""
    rng = np.random.default_rng(4)
    for n in (1, 63, 64, 65, 129):
        rows = small_rows(n, dtype, rng)
        data, offsets = device_rows(rows, dtype)
        check(rows, data, offsets, spans_from_lists(short_spans(rows, rng), lead=3), "n_rows %d" % n, behind=5)
    rows = small_rows(192, dtype, rng)
    per_row = short_spans(rows, rng)
    per_row[64:128] = [[] for _ in range(64)]
    data, offsets = device_rows(rows, dtype)
    check(rows, data, offsets, spans_from_lists(per_row, lead=3), "a group without spans", behind=5)
    check(rows, data, offsets, spans_from_lists([[] for _ in rows], lead=3), "no spans at all", behind=5)
    rows = small_rows(65, dtype, rng)
    rows[64] = rng.choice(np.array([97, 98]), 40).astype(dtype)
    per_row = [[] for _ in rows]
    per_row[64] = short_spans([rows[64]] * 70, rng, per_row=1, max_len=6)
    per_row[64] = [x[0] for x in per_row[64]]
    data, offsets = device_rows(rows, dtype)
    check(rows, data, offsets, spans_from_lists(per_row, lead=3), "spans in row 64 only", behind=5)
    rows = small_rows(3, dtype, rng)
    rows[1] = rng.choice(np.array([97, 98, 99]), 300).astype(dtype)
    per_row = [[(0, 1)], [x[0] for x in short_spans([rows[1]] * 1000, rng, per_row=1, max_len=7)], [(0, 2)]]
    data, offsets = device_rows(rows, dtype)
    first, count = check(rows, data, offsets, spans_from_lists(per_row, lead=3), "1000 spans in one row", behind=5)
    assert 100 < int((first[3:1005] == np.arange(3, 1005)).sum()) < 1000


_bits_case = {}


def bits_case(dtype):
    """About 2000 spans over a two-letter alphabet and 200 distinct longer texts, each of them twice."""
    if dtype not in _bits_case:
        rng = np.random.default_rng(5)
        rows = small_rows(500, dtype, rng, max_len=10)
        per_row = [[(s, min(e, len(row))) for s, e in mine] for row, mine in zip(rows, short_spans(rows, rng, per_row=4, max_len=6))]
        for k in range(200):
            text = np.concatenate([rng.integers(1, 250, int(rng.integers(20, 60))), [k + 1, 251]]).astype(dtype)  # (pairwise distinct: k)
            for _ in range(2):
                r = int(rng.integers(0, len(rows)))
                at = len(rows[r])
                rows[r] = np.concatenate([rows[r], text])
                per_row[r].append((at, at + text.size))
        spans = spans_from_lists(per_row, lead=3)
        data, offsets = device_rows(rows, dtype)
        want = group_ref(rows, spans, S_FIRST, S_COUNT)
        assert len(spans[1]) == 3 + 2000 + 400
        _bits_case[dtype] = (rows, spans, data, offsets, want)
    return _bits_case[dtype]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("hash_bits", [64, 16, 8, 1, 0])
def test_every_hash_width_gives_the_same_arrays(dtype, hash_bits):
    """hash_bits 64, 16, 8, 1, 0: identical to the model.  At 0 every span walks ONE probe chain past every distinct text filed before
    it -- 282 texts, 2400 spans, each past half of the texts on average: about 3 x 10^5 slot visits with a text comparison -- and only
    that comparison tells them apart: the exactness test."""
    rows, spans, data, offsets, (want_f, want_c) = bits_case(dtype)
    rc, status, first, count = run_group(data, offsets, spans, hash_bits=hash_bits)
    assert (rc, status) == (0, 0)
    bad = np.nonzero((first != want_f) | (count != want_c))[0]
    assert bad.size == 0, (hash_bits, bad[:10], first[bad[:5]], want_f[bad[:5]], count[bad[:5]], want_c[bad[:5]])
    lo = int(spans[0][0])
    leaders = int((first[lo:] == np.arange(lo, first.size)).sum())
    assert 200 + 60 < leaders < 200 + 2 ** 7 and (count[lo:] >= 1).all()


@pytest.mark.parametrize("dtype", DTYPES)
def test_contention(dtype):
    """5000 spans of one text -- one slot, one count, every wave at it: first == M0 everywhere, count == 5000 -- and 5000 pairwise
    distinct texts: every span its own leader."""
    rng = np.random.default_rng(6)
    word = np.array([110, 101, 101, 100, 108, 101], dtype)
    rows, per_row = [], []
    for r in range(100):
        pads = rng.integers(0, 5, 50)
        rows.append(np.concatenate([np.concatenate([rng.integers(1, 100, int(p)).astype(dtype), word]) for p in pads]))
        at = np.cumsum(pads + word.size) - word.size
        per_row.append([(int(a), int(a) + word.size) for a in at])
    data, offsets = device_rows(rows, dtype)
    spans = spans_from_lists(per_row, lead=3)
    first, count = check(rows, data, offsets, spans, "one text", behind=5)
    assert (first[3:5003] == 3).all() and (count[3:5003] == 5000).all()
    rows = [np.concatenate([np.frombuffer(b"%04d" % (50 * r + k), np.uint8) for k in range(50)]).astype(dtype) for r in range(100)]
    per_row = [[(4 * k, 4 * k + 4) for k in range(50)] for _ in rows]
    data, offsets = device_rows(rows, dtype)
    first, count = check(rows, data, offsets, spans_from_lists(per_row, lead=3), "all distinct", behind=5)
    assert (first[3:5003] == np.arange(3, 5003)).all() and (count[3:5003] == 1).all()


@pytest.mark.parametrize("dtype", DTYPES)
def test_long_spans(dtype):
    """Two 5000-unit spans equal but for unit 4999, and a third equal to the first, at different alignments."""
    rng = np.random.default_rng(7)
    a = rng.integers(1, 250, 5000).astype(dtype)
    b = a.copy()
    b[4999] ^= 1
    rows = [np.concatenate([[7], a]).astype(dtype), np.concatenate([[7, 7, 7], b, [9]]).astype(dtype), np.concatenate([[7] * 6, a, a[:5]]).astype(dtype)]
    spans = spans_from_lists([[(1, 5001)], [(3, 5003)], [(6, 5006)]], lead=3)
    data, offsets = device_rows(rows, dtype)
    for hash_bits in (64, 0):
        first, count = check(rows, data, offsets, spans, "long", hash_bits=hash_bits, behind=5)
        assert first[3:6].tolist() == [3, 4, 3] and count[3:6].tolist() == [2, 1, 2]


@pytest.mark.parametrize("dtype", DTYPES)
def test_malformed_and_absent_spans(dtype):
    """random_spans -- out-of-row, reversed, overlapping and repeated spans, every length class and alignment -- are grouped by their
    clamped text; absent spans mixed in get NEEDLE_GROUP_NONE / 0 and change nobody's count."""
    rng = np.random.default_rng(8)
    cw = np.dtype(dtype).itemsize
    rows = [rng.choice(np.array([97, 98]), int(k)).astype(dtype) for k in rng.integers(16, 50, 80)] + small_rows(20, dtype, rng)
    data, offsets = device_rows(rows, dtype)
    off, start, end = random_spans(rows, rng, abs0=int(offsets[0]), cw=cw, lead=3)
    plain = (off, start.copy(), end.copy())
    first0, count0 = check(rows, data, offsets, plain, "malformed", behind=5)
    gone = np.nonzero(rng.random(start.size) < 0.2)[0]
    gone = gone[gone >= 3]
    start[gone], end[gone] = -1 - rng.integers(0, 9, gone.size).astype(np.int32), -1 - rng.integers(0, 9, gone.size).astype(np.int32)
    first, count = check(rows, data, offsets, (off, start, end), "absent", behind=5)
    assert gone.size > 50 and (first[gone] == NONE).all() and (count[gone] == 0).all()
    # nobody's count holds an absent span: the counts of the groups add up to the spans that are present
    lo, hi = int(off[0]), int(off[-1])
    leaders = lo + np.nonzero(first[lo:hi] == np.arange(lo, hi))[0]
    absent = (start[lo:hi] < 0) & (end[lo:hi] < 0)  # (random_spans' own (-7, -2) among them)
    assert int(count[leaders].sum()) == hi - lo - int(absent.sum()) and int(absent.sum()) >= gone.size
    leaders0 = lo + np.nonzero(first0[lo:hi] == np.arange(lo, hi))[0]
    assert int(count0[leaders0].sum()) > int(count[leaders].sum())


def test_overflow_and_the_table_at_its_minimum():
    """max_spans below the device-side count: status 1, NEEDLE_OK, the call terminates and nothing outside [M0, M1) is written.
    max_spans at exactly the count (64 spans in 128 slots, 32 in 64: the table at its minimum size, half full): status 0, the model."""
    from needle_amd import _lib
    rng = np.random.default_rng(9)
    for n_spans in (64, 32, 1000):
        rows = small_rows(n_spans // 2, np.uint8, rng, alphabet=(97, 98, 99, 100), max_len=20)
        spans = spans_from_lists(short_spans(rows, rng, per_row=2, max_len=12), lead=3)
        data, offsets = device_rows(rows, np.uint8)
        assert int(_lib.lib().needle_group_spans_work_bytes(n_spans)) < int(_lib.lib().needle_group_spans_work_bytes(2 * n_spans))
        check(rows, data, offsets, spans, "exactly the count", behind=5, max_spans=n_spans)
        for max_spans in (n_spans - 1, n_spans // 2, 1, 0):
            rc, status, first, count = run_group(data, offsets, spans, behind=5, max_spans=max_spans)
            assert (rc, status) == (0, 1), (n_spans, max_spans, rc, status)
            for a, s in ((first, S_FIRST), (count, S_COUNT)):
                assert (a[:3] == s).all() and (a[3 + n_spans:] == s).all(), (n_spans, max_spans)
    # both lists NULL with max_spans == 0: an empty list is fine, a list that claims spans raises the status
    rows = small_rows(70, np.uint8, rng)
    data, offsets = device_rows(rows, np.uint8)
    rc, status, first, count = run_group(data, offsets, spans_from_lists([[] for _ in rows]), max_spans=0, null_lists=True, behind=4)
    assert (rc, status) == (0, 0) and (first == S_FIRST).all() and (count == S_COUNT).all()
    claims = spans_from_lists([[(0, 1)] for _ in rows])
    rc, status, first, count = run_group(data, offsets, (claims[0], claims[1][:0], claims[2][:0]), max_spans=0, null_lists=True, behind=4)
    assert (rc, status) == (0, 1) and (first == S_FIRST).all() and (count == S_COUNT).all()
    # an empty batch stores status 0
    rc, status, first, count = run_group(data, offsets, spans_from_lists([[(0, 1)]]), n_rows=0, behind=4)
    assert (rc, status) == (0, 0) and (first == S_FIRST).all() and (count == S_COUNT).all()


def test_determinism_on_two_streams():
    """The same call three times on the default stream and three times on a second one: identical arrays."""
    import torch
    rows, spans, data, offsets, (want_f, want_c) = bits_case(np.uint8)
    other = torch.cuda.Stream()
    torch.cuda.synchronize()
    for stream in (None, other):
        for _ in range(3):
            rc, status, first, count = run_group(data, offsets, spans, stream=stream)
            assert (rc, status) == (0, 0) and (first == want_f).all() and (count == want_c).all()


def test_python_group_spans_packed():
    """Pattern.group_spans_packed on device tensors and on numpy inputs: int64 / int32 results indexed like start, -1 / 0 outside the
    list and for absent spans; a list that claims more spans than start holds raises."""
    import torch
    from needle_amd.pattern import DeviceError, Pattern
    rows, spans, data, offsets, (want_f, want_c) = bits_case(np.uint16)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to("cuda")
    off, start, end = spans
    start, end = start.copy(), end.copy()
    start[10], end[10] = -1, -4
    want_f, want_c = group_ref(rows, (off, start, end), NONE, 0)
    for bits in (64, 3):
        first, count = Pattern.group_spans_packed(data, offsets, dev(off), dev(start), dev(end), hash_bits=bits)
        assert first.is_cuda and first.dtype == torch.int64 and count.dtype == torch.int32 and first.numel() == count.numel() == start.size
        assert (first.cpu().numpy().view(np.uint64) == want_f).all() and (count.cpu().numpy().view(np.uint32) == want_c).all()
    assert int(first[10]) == -1 and int(first[0]) == -1 and int(count[10]) == 0
    host = np.concatenate(rows)
    host_off = np.concatenate([[0], np.cumsum([len(r) for r in rows])])
    first, count = Pattern.group_spans_packed(host, host_off, off, start, end)
    assert isinstance(first, np.ndarray) and (first.view(np.uint64) == want_f).all() and (count.view(np.uint32) == want_c).all()
    claims = off - 3  # (the list without its foreign entries, and two spans more than start / end hold)
    claims[-1] += 2
    with pytest.raises(DeviceError):
        Pattern.group_spans_packed(data, offsets, dev(claims), dev(start[3:]), dev(end[3:]))
    with pytest.raises(DeviceError, match="status 1"):  # an empty start / end under offsets that claim spans
        Pattern.group_spans_packed(data, offsets, dev(claims), dev(start[:0]), dev(end[:0]))
    empty = torch.zeros(off.size, dtype=torch.int64, device="cuda")
    first, count = Pattern.group_spans_packed(data, offsets, empty, dev(start[:0]), dev(end[:0]))
    assert first.numel() == 0 and count.numel() == 0 and first.dtype == torch.int64 and count.dtype == torch.int32


def counter_of_matches(p, strings):
    c = collections.Counter()
    for s, spans in zip(strings, p.find_all_strings(strings)):
        u = s.encode("utf-16-le", "surrogatepass")
        for a, b in spans:
            c[u[2 * a:2 * b].decode("utf-16-le", "surrogatepass")] += 1
    return list(c.items())  # (insertion order: first occurrence)


def test_count_distinct_strings_on_the_must_work_patterns():
    """count_distinct_strings against collections.Counter over the library's own find_all_strings slices, on the thirteen patterns of
    captures_cases.MUST_WORK and their texts, repeated and joined so that matches recur within and across rows."""
    from captures_cases import MUST_WORK
    from needle_amd.pattern import DFACompiler
    assert len(MUST_WORK) == 13
    some = 0
    for regex, flags, _, texts in MUST_WORK:
        p = DFACompiler.compile(regex, flags=flags)
        strings = list(texts) + [" ".join(texts), ""] + list(reversed(texts)) + [t + ";" + t for t in texts]
        want = counter_of_matches(p, strings)
        assert p.count_distinct_strings(strings) == want, regex
        some += len(want) > 1 and any(k > 1 for _, k in want)
    assert some >= 8


def test_count_distinct_group_strings():
    """Group g of every match, grouped: on ([0-9]+)-([0-9]+), and on (a(b)?)+ whose group 2 is optional -- the matches that did not pass
    it are absent and are not reported."""
    from needle_amd.pattern import DFACompiler
    cases = [(r"([0-9]+)-([0-9]+)", ["1-2 3-2", "10-2", "1-22 1-2", "", "x", "7-7 7-7 10-7"]), (r"(a(b)?)+", ["aba", "a", "ab ab", "b a", "abab aa", "", "ba"])]
    absent = 0
    for regex, strings in cases:
        p = DFACompiler.compile(regex)
        groups = p.find_all_groups_strings(strings)
        for g in range(p.group_count() + 1):
            c = collections.Counter()
            for s, matches in zip(strings, groups):
                for m in matches:
                    if m[g] is None:
                        absent += 1
                    else:
                        c[s[m[g][0]:m[g][1]]] += 1
            assert p.count_distinct_group_strings(strings, g) == list(c.items()), (regex, g)
    assert absent >= 3


def test_count_distinct_bytes_with_ill_formed_input():
    """UTF-8 rows, some ill-formed: the byte positions of find_all_utf8_packed grouped on the ORIGINAL bytes."""
    from needle_amd.pattern import DFACompiler
    p = DFACompiler.compile("[0-9]+|é+|[а-я]+")
    rows = ["12 é 12".encode(), b"\xff12\xfe 7", "привет 12 éé привет".encode(), b"", "é".encode() + b"\xc3 7 \xe2\x82", b"12\x80\x8012", "ééé é".encode()]
    c = collections.Counter()
    for row, spans in zip(rows, p.find_all_bytes(rows)):
        for a, b in spans:
            c[row[a:b]] += 1
    got = p.count_distinct_bytes(rows)
    assert got == list(c.items()) and dict(got)[b"12"] >= 5 and "é".encode() in dict(got)


def test_distinct_rows_through_lines_packed():
    """300 lines with repeats, cut by lines_packed, then distinct_rows_packed: uniq -c of the lines in first-occurrence order, and
    every line's group."""
    import torch
    from needle_amd.pattern import Pattern, lines_packed
    rng = np.random.default_rng(10)
    pool = [b"GET /index.html 200", b"", b"POST /login 302", b"GET /index.html 404", b"GET /a 200", b"x"] + [b"line %d" % i for i in range(40)]
    lines = [pool[int(i)] for i in rng.integers(0, len(pool), 300)]
    buf = np.frombuffer(b"\n".join(lines) + b"\n", np.uint8)
    data = torch.from_numpy(np.concatenate([buf, np.zeros(4 + (-buf.size) % 4, np.uint8)])).to("cuda")
    text, line_off, _ = lines_packed(data[:buf.size])
    assert line_off.numel() == 301
    dtext, doff, counts, gid = Pattern.distinct_rows_packed(text, line_off)
    torch.cuda.synchronize()
    c = collections.Counter(lines)
    dtext, doff = dtext.cpu().numpy(), doff.cpu().numpy()
    got = [(dtext[doff[g]:doff[g + 1]].tobytes(), int(k)) for g, k in enumerate(counts.cpu().numpy())]
    assert got == list(c.items()) and len(got) < 60
    keys = list(c)
    assert gid.cpu().numpy().tolist() == [keys.index(x) for x in lines]


def test_distinct_text_stays_on_the_device_for_the_next_entry():
    """distinct_spans_packed on a match list; its (text, offsets) goes into contained_in_packed as it is: the keywords that hold a digit."""
    import torch
    from needle_amd.pattern import DFACompiler, Pattern, unpack_bitmap
    words = ["alpha", "beta7", "gamma", "d3lta", "beta7", "alpha", "x9", "gamma", "alpha"]
    rows = [np.frombuffer((" ".join(words[i:] + words[:i])).encode(), np.uint8) for i in range(len(words))]
    data, offsets = device_rows(rows, np.uint8)
    p, digit = DFACompiler.compile("[a-z0-9]+"), DFACompiler.compile("[0-9]")
    off, st, en = p.find_all_packed(data, offsets)
    text, toff, counts, gid = Pattern.distinct_spans_packed(data, offsets, off, st, en)
    assert text.is_cuda and toff.is_cuda and counts.is_cuda and gid.is_cuda
    bits = digit.contained_in_packed(text, toff)
    torch.cuda.synchronize()
    order = list(dict.fromkeys(words))
    host, ho = text.cpu().numpy(), toff.cpu().numpy()
    assert [host[ho[g]:ho[g + 1]].tobytes().decode() for g in range(len(order))] == order
    assert counts.cpu().numpy().tolist() == [words.count(w) * len(words) for w in order]
    assert unpack_bitmap(bits, len(order)).tolist() == [any(ch.isdigit() for ch in w) for w in order]
    assert gid.cpu().numpy()[:len(words)].tolist() == [order.index(w) for w in words]
    # the numpy form gives the same table
    host_data, host_off = np.concatenate(rows), np.concatenate([[0], np.cumsum([len(r) for r in rows])])
    t2, o2, c2, g2 = p.distinct_matches_packed(host_data, host_off)
    assert isinstance(t2, np.ndarray) and t2.tobytes() == host[:ho[-1]].tobytes() and (o2 == ho).all() and (c2 == counts.cpu().numpy()).all()


def test_fuzz():
    """100 seeded batches of rows over small alphabets with random_spans' lists (every alignment, malformed spans) and some absent
    spans, at random hash_bits and both widths: all of them run -- the entry never sees a pattern, so nothing can refuse."""
    ran = 0
    for seed in range(100):
        rng = np.random.default_rng(1000 + seed)
        dtype = DTYPES[seed % 2]
        cw = np.dtype(dtype).itemsize
        alphabet = np.array([97, 98, 0][:int(rng.integers(1, 4))] if seed % 3 else [97, 0x161, 98][:2 + cw - 1])
        n = int(rng.integers(17, 70))
        rows = [rng.choice(alphabet, int(k)).astype(dtype) for k in rng.integers(16, 40, n)]
        if seed % 4 == 0:
            rows += small_rows(int(rng.integers(1, 80)), dtype, rng, alphabet=alphabet)
        data, offsets = device_rows(rows, dtype, seed=seed)
        off, start, end = random_spans(rows, rng, abs0=int(offsets[0]), cw=cw, lead=int(rng.integers(0, 4)))
        gone = np.nonzero(rng.random(start.size) < 0.05)[0]
        gone = gone[gone >= int(off[0])]
        start[gone], end[gone] = -1, -1 - (seed % 3)
        hash_bits = int(rng.choice([64, 64, 32, 12, 6, 3, 1, 0]))
        check(rows, data, offsets, (off, start, end), ("fuzz", seed), hash_bits=hash_bits, behind=int(rng.integers(0, 4)))
        ran += 1
    assert ran == 100
