"""The n-gram candidate filter in front of PACKED row batches (needle_amd/csrc/needle_ngram_packed.h), host side: the algorithm on packed
streams, restated with tests/prefilter_sim.py on the reference-layout tables against the CPU oracle.  A packed batch is one stream of
code units; the kernel samples one window every S chars at FIXED positions of the stream -- multiples of S counted from a 16-aligned base
in front of the text -- so a row that starts at stream position s sees its windows end at row-relative positions = -s (mod S): "some
phase" per row, which the filter's bitmap does not depend on.  A window that does not lie wholly inside its row is dropped (its end is
fewer than 4 chars into the row); a keyword split over two adjacent rows therefore makes no candidate that could match, and the verify
walk of a window never leaves its row.  No GPU needed."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CHILD = r'''
import sys, numpy as np
sys.path.insert(0, "."); sys.path.insert(0, "tests")
from needle_amd import workload as W
from needle_amd.pattern import DFACompiler
from test_compile_matches_txt import oracle_for
import prefilter_sim as sim
from oracle import walker
walker.build()
rng = np.random.default_rng(11)


def packed_batch(words, alpha, n_rows):
    """Rows of ragged lengths with keywords planted whole, cut, at both ends; empty rows, rows of 1..3 chars, a keyword as a whole row, two
    adjacent one-keyword rows, and a keyword SPLIT over rows r / r + 1 (which must not match)."""
    rows = []
    for r in range(n_rows):
        kind = r % 12
        w = [ord(c) for c in words[int(rng.integers(0, len(words)))]]
        fill = lambda n: list(rng.choice(alpha, size=n))
        if kind == 0:
            rows.append([])
        elif kind == 1:
            rows.append(fill(int(rng.integers(1, 4))))
        elif kind == 2:
            rows.append(w)                                    # the keyword is the whole row
        elif kind == 3:
            rows.append(w)                                    # ... and so is its neighbour
        elif kind == 4:
            cut = int(rng.integers(1, len(w)))
            rows.append(fill(int(rng.integers(0, 20))) + w[:cut])   # split: head at this row's end ...
            rows.append(w[cut:] + fill(int(rng.integers(0, 20))))   # ... tail at the next row's start
        elif kind == 5:
            rows.append(w + fill(int(rng.integers(0, 30))))   # at the row's first chars
        elif kind == 6:
            rows.append(fill(int(rng.integers(0, 30))) + w)   # at its last chars
        elif kind == 7:
            rows.append(fill(int(rng.integers(0, 30))) + w[:-1])  # cut by the row's end
        else:
            n = int(rng.integers(0, 70))
            t = fill(n)
            if n > len(w) and kind < 10:
                at = int(rng.integers(0, n - len(w) + 1))
                t[at:at + len(w)] = w
            rows.append(t)
    return rows


def check(rx, rows, lead, want_on2=None, want_fixed=False):
    p = DFACompiler.compile(rx, "t", 0)
    o, _ = oracle_for(rx, 0)
    fi, ci = p.prefilter_info("forwards", with_bitmap=True), p.prefilter_info("contained_in", with_bitmap=True)
    assert fi["on"] and ci["on"], (rx[:40], fi.get("why"), ci.get("why"))
    if want_on2 is not None:
        assert fi["on2"] == want_on2, fi["on2"]
    if want_fixed:
        assert p.tables()["fixed_len"] >= 0
    # the stream: `lead` chars of something else in front of offsets[0] (the 16-aligned base lies `lead` chars ahead of the text)
    offsets = np.cumsum([lead] + [len(r) for r in rows])
    n_match = n_split = 0
    for r, row in enumerate(rows):
        text = np.array(row, dtype=np.uint8)
        start = int(offsets[r])                      # the row's first char as a stream position
        want = o.find_all(text)[:1]
        exp = ((True,) + want[0]) if want else (False, -1, -1)
        # sampled stream positions = 0 (mod S) -> row-relative window ends = -start (mod S); ends < 4 are dropped by sim.filtered
        got = sim.filtered(p, "find", text, info=fi, phase=(-start) % fi["stride"])
        assert got == exp, (rx[:40], r, start, bytes(text), got, exp)
        got_c = sim.filtered(p, "contained_in", text, info=ci, phase=(-start) % ci["stride"])
        assert got_c[0] == bool(want), (rx[:40], r, start, bytes(text))
        n_match += bool(want)
    return n_match


alpha = [ord(c) for c in "abcdefghijklmnopqrstuvwxyz "]
total = 0
# 300 keywords of 6..8 chars
words = W.keywords(300, min_len=6, max_len=8)
rows = packed_batch(words, alpha, 240)
for lead in (0, 3, 13):
    total += check("|".join(words), rows, lead)
# a dictionary whose shortest match is one char too short for the plain second level: the TWO-SIDED one (on2 == 2)
names = ["Sherlock", "Holmes", "Watson", "Irene", "Adler", "Baker"]
rows = packed_batch(names, [ord(c) for c in "SherlockHmsWatnIdB xyz"], 240)
for lead in (0, 1, 6):
    total += check("|".join(names), rows, lead, want_on2=2)
# one length: start = end - 8
rows = packed_batch(["abcdefgh"], [ord(c) for c in "abcdefgh x"], 240)
for lead in (0, 5):
    total += check("abcdefgh", rows, lead, want_fixed=True)
assert total > 300, total
# a keyword split over two adjacent rows matches in neither (and does when the rows are one)
p = DFACompiler.compile("abcdefgh", "t", 0)
fi = p.prefilter_info("forwards", with_bitmap=True)
for cut in range(1, 8):
    for start in range(0, 4):
        a, b = np.frombuffer(b"xy" + b"abcdefgh"[:cut], dtype=np.uint8), np.frombuffer(b"abcdefgh"[cut:] + b"zz", dtype=np.uint8)
        assert sim.filtered(p, "find", a, info=fi, phase=(-start) % fi["stride"]) == (False, -1, -1)
        assert sim.filtered(p, "find", b, info=fi, phase=(-(start + len(a))) % fi["stride"]) == (False, -1, -1)
        assert sim.filtered(p, "find", np.concatenate([a, b]), info=fi, phase=(-start) % fi["stride"]) == (True, 2, 10)
print("PACKED-PREFILTER-SIM-OK", total)
'''


def test_filter_algorithm_on_packed_streams_vs_oracle():
    """NEEDLE_PREFILTER=2 builds filters for plain LDS-table automata too (read once per process: a child)."""
    env = dict(os.environ, NEEDLE_PREFILTER="2", NEEDLE_PAIR_MAX_BYTES="0")
    r = subprocess.run([sys.executable, "-c", CHILD], env=env, capture_output=True, text=True, timeout=1500, cwd=ROOT)
    assert "PACKED-PREFILTER-SIM-OK" in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]
