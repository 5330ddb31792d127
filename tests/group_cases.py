"""The model of needle_group_spans_packed_dev for its tests (test_group_abi.py on the CPU, test_gpu_group.py on the GPU): clamp, slice,
a dict of first index and count.  A span list is (span_offsets int64[n_rows + 1], start int32[M], end int32[M]) as in set_spans_cases.py;
rows are str, bytes or 1-D numpy arrays of code units."""
import numpy as np

NONE = 0xFFFFFFFFFFFFFFFF  # NEEDLE_GROUP_NONE


def clamp_span(s, e, n):
    s = min(max(int(s), 0), n)
    return s, min(max(int(e), s), n)


def span_text(row, s, e):
    """The clamped text of a span as a hashable value."""
    s, e = clamp_span(s, e, len(row))
    t = row[s:e]
    return t.tobytes() if isinstance(t, np.ndarray) else t


def group_ref(rows, spans, fill_first=NONE, fill_count=0):
    """(first uint64[M], count uint32[M]): what the entry must write for m in [span_offsets[0], span_offsets[n]); the entries outside
    hold fill_first / fill_count (the tests' sentinels).  A span with start < 0 and end < 0 is absent: NONE / 0."""
    off, start, end = spans
    first = np.full(len(start), fill_first, np.uint64)
    count = np.full(len(start), fill_count, np.uint32)
    seen = {}  # text -> [first index, count]
    key = {}
    for r, row in enumerate(rows):
        for m in range(int(off[r]), int(off[r + 1])):
            if start[m] < 0 and end[m] < 0:
                key[m] = None
                continue
            t = span_text(row, start[m], end[m])
            key[m] = t
            if t in seen:
                seen[t][0] = min(seen[t][0], m)
                seen[t][1] += 1
            else:
                seen[t] = [m, 1]
    for m, t in key.items():
        first[m], count[m] = (NONE, 0) if t is None else seen[t]
    return first, count


def distinct_ref(rows, spans):
    """[(text, count)] in first-occurrence order: the table distinct_spans_packed must give."""
    first, count = group_ref(rows, spans)
    off, start, end = spans
    row_of = np.repeat(np.arange(len(rows)), np.diff(off))
    lo = int(off[0])
    return [(span_text(rows[row_of[m - lo]], start[m], end[m]), int(count[m])) for m in range(lo, int(off[-1])) if first[m] == m]
