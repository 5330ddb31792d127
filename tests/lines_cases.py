"""The reference of the line splitter (needle_lines_count_packed_dev / needle_lines_fill_packed_dev; lines_packed): the rule of
include/needle_hip.h written out unit by unit, and the packed batch it gives for a list of documents.  tests/test_lines_abi.py pins it to
bytes.splitlines; every GPU test of the feature compares against it bit for bit."""
import numpy as np

LF, CR = 0x0A, 0x0D


def lines_ref(units, keep):
    """The lines of ONE document (any sequence of code units) -> list of lists of ints.  Unit i is a line's last unit iff it is '\\n', or
    '\\r' not followed by '\\n' within the document, or the document's last unit and no terminator.  keep: the lines with their
    terminators; else without any terminator unit."""
    u = [int(x) for x in units]
    n = len(u)
    lines, start = [], 0
    for i in range(n):
        if u[i] == LF or (u[i] == CR and not (i + 1 < n and u[i + 1] == LF)) or (i == n - 1 and u[i] != LF and u[i] != CR):
            line = u[start:i + 1]
            lines.append(line if keep else [x for x in line if x != LF and x != CR])
            start = i + 1
    assert start == n
    return lines


def batch_ref(docs, keep, dtype):
    """The lines of a batch of documents -> (text, line_offsets int64[lines + 1] from 0, doc_line_offsets int64[n + 1]).  keep: text is the
    documents back to back, as the input span is."""
    lines, doc_off = [], [0]
    for d in docs:
        lines += lines_ref(d, keep)
        doc_off.append(len(lines))
    off = np.zeros(len(lines) + 1, np.int64)
    if lines:
        off[1:] = np.cumsum([len(l) for l in lines])
    text = np.array([x for l in lines for x in l], dtype=dtype)
    return text, off, np.array(doc_off, np.int64)


def tile_counts_ref(docs, lead, tile_units, tiles):
    """Per tile of `tile_units` units: (events, kept units), the documents lying back to back from unit `lead` of the data."""
    _, off, _ = batch_ref(docs, True, np.int64)
    events = off[1:] - 1 + lead
    flat = np.array([int(x) for d in docs for x in d], np.int64)
    kept = np.nonzero((flat != LF) & (flat != CR))[0] + lead
    count = lambda pos: np.bincount(pos // tile_units, minlength=tiles)[:tiles].astype(np.int64)
    return count(events), count(kept)
