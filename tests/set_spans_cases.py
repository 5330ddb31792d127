"""Span lists and their reference answers for the tests of needle_set_matches_spans_packed_dev (test_set_spans_abi.py on the CPU,
test_gpu_set_spans.py on the GPU).  A span list is (span_offsets int64[n_rows + 1], start int32[M], end int32[M]): row r's spans are
start / end[span_offsets[r] : span_offsets[r + 1]], relative to the row; span_offsets[0] may be > 0 (the entries below it are nobody's)."""
import numpy as np

from pattern_set_cases import GPU_RECIPE, SETS, gpu_batch, set_flags, split_case


def clamp_span(s, e, n):
    """The entry's clamp: s' = clamp(s, 0, len), e' = clamp(e, s', len)."""
    s = min(max(int(s), 0), n)
    return s, min(max(int(e), s), n)


def reference_span_masks(oracles, rows, spans):
    """uint32[M]: bit i of entry m = member i's oracle matches() on the clamped substring of span m's row (entries outside
    [span_offsets[0], span_offsets[n]) stay 0)."""
    off, start, end = spans
    out = np.zeros(len(start), np.uint32)
    for r, row in enumerate(rows):
        for m in range(int(off[r]), int(off[r + 1])):
            s, e = clamp_span(start[m], end[m], len(row))
            sub = np.ascontiguousarray(row[s:e])
            bits = 0
            for i, o in enumerate(oracles):
                if o.matches(sub):
                    bits |= 1 << i
            out[m] = bits
    return out


def spans_from_lists(per_row, lead=0):
    """[[(s, e), ...] per row] -> a span list whose first `lead` entries belong to no row."""
    off = np.zeros(len(per_row) + 1, np.int64)
    off[0] = lead
    off[1:] = lead + np.cumsum([len(x) for x in per_row])
    flat = [se for x in per_row for se in x]
    start = np.array([0] * lead + [s for s, _ in flat], dtype=np.int32)
    end = np.array([0] * lead + [e for _, e in flat], dtype=np.int32)
    return off, start, end


def union_regex(name):
    return "|".join("(" + p + ")" for p in SETS[name][0])


# Members that no union span can carry.  The reference's alternation is ordered (the first alternative that matches at the leftmost
# start wins, not the longest): every match of logs8's member 7 "a.c" begins with an "a", which member 6 "(ab|a|bcdef|g)+" matches
# first -- the union's span there is the "a" alone, (0, 1) of "a-c".  A property of the reference; the member's bit is
# covered by the whole-row and the arbitrary spans.
SHADOWED = {"logs8": {7}}

_union = {}


def union_spans(case):
    """(rows, span list): the oracle's find_all of the set's union pattern (compiled with the set's flags) over the set's gpu_batch,
    computed once per "name" or "name@8" / "name@16" (pattern_set_cases.split_case)."""
    if case not in _union:
        from test_compile_matches_txt import oracle_for
        name, dtype = split_case(case)
        o = oracle_for(union_regex(name), set_flags(name))[0]
        rows = gpu_batch(name, dtype=dtype, **GPU_RECIPE.get(name, {}))
        _union[case] = (rows, spans_from_lists([o.find_all(np.ascontiguousarray(r)) for r in rows]))
    return _union[case]


SPAN_LENGTHS = [0, 1, 15, 16, 17, 31, 32, 33]
MALFORMED = [(-5, 3), (2, 10 ** 6), (9, 4), (-7, -2), (10 ** 6, 10 ** 6 + 5), (3, -1)]  # negative s, e > len, e < s


def random_spans(rows, rng, abs0=0, cw=1, lead=0):
    """Arbitrary spans of `rows` (row r's text begins at absolute code unit abs0 + sum of the earlier lengths): per row with text the
    lengths of SPAN_LENGTHS that fit and the whole row, at random starts; over the batch every alignment 0 .. 15 of the span's first
    absolute byte at least once (asserted); the spans of a row in random order (unordered, overlapping); the MALFORMED spans in turn,
    one per row."""
    per_row, seen = [], set()
    at = abs0
    for r, row in enumerate(rows):
        n = len(row)
        mine = [(0, n)]
        for L in SPAN_LENGTHS:
            if L <= n:
                s = int(rng.integers(0, n - L + 1))
                mine.append((s, s + L))
        if n >= 16:  # an alignment of the first absolute byte, in turn
            want = (r % 16) // cw * cw
            s = next(s for s in range(16) if ((at + s) * cw) % 16 == want)
            if s < n:
                mine.append((s, int(rng.integers(s, n + 1))))
        mine.append(MALFORMED[r % len(MALFORMED)])
        order = rng.permutation(len(mine))
        mine = [mine[i] for i in order]
        for s, e in mine:
            cs, ce = clamp_span(s, e, n)
            if ce > cs:
                seen.add(((at + cs) * cw) % 16)
        per_row.append(mine)
        at += n
    assert seen == set(range(0, 16, cw)), sorted(seen)
    return spans_from_lists(per_row, lead)
