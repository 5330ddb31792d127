"""The references of the gather entries (needle_gather_spans_*_packed_dev, needle_split_spans_packed_dev; include/needle_hip.h): what a
span list extracts from its rows and what a match list splits them into, by the definitions' own words.  tests/test_gather_abi.py pins
them to hand-written answers and to CPython's re; tests/test_gpu_gather.py compares the device against them bit for bit."""
import numpy as np


def clamp_span(s, e, n):
    """(s', e'): s' = clamp(s, 0, n), e' = clamp(e, s', n)."""
    s = min(max(int(s), 0), n)
    return s, min(max(int(e), s), n)


def gather_ref(rows, lists):
    """Per row the list of row[s':e'] for its spans, in list order.  Works on str and numpy rows alike."""
    out = []
    for row, spans in zip(rows, lists):
        got = []
        for s, e in spans:
            s, e = clamp_span(s, e, len(row))
            got.append(row[s:e])
        out.append(got)
    return out


def split_list_ref(rows, lists):
    """Per row the complement of its match list: c matches give c + 1 pieces; piece k starts at 0 (k = 0) or at e'_(k-1), ends at len (k = c)
    or at s'_k, the end raised to at least the start."""
    out = []
    for row, spans in zip(rows, lists):
        n, c = len(row), len(spans)
        cl = [clamp_span(s, e, n) for s, e in spans]
        pieces = []
        for k in range(c + 1):
            ps = 0 if k == 0 else cl[k - 1][1]
            pe = n if k == c else cl[k][0]
            pieces.append((ps, max(pe, ps)))
        out.append(pieces)
    return out


def flatten(lists):
    """Per-row lists of (s, e) -> the CSR triple (offsets int64[n + 1], start int32, end int32)."""
    off = np.zeros(len(lists) + 1, np.int64)
    off[1:] = np.cumsum([len(x) for x in lists])
    st = np.array([s for x in lists for s, _ in x], np.int32)
    en = np.array([e for x in lists for _, e in x], np.int32)
    return off, st, en


def packed_ref(rows, lists, dtype):
    """gather_ref as a packed batch: (text, offsets from 0, span offsets)."""
    parts = [np.asarray(x, dtype) for per in gather_ref([np.asarray(r, dtype) for r in rows], lists) for x in per]
    off = np.zeros(len(parts) + 1, np.int64)
    off[1:] = np.cumsum([x.size for x in parts])
    text = np.concatenate(parts).astype(dtype) if parts else np.zeros(0, dtype)
    return text, off, flatten(lists)[0]
