"""Packed-mode matches() / containedIn() keep two 64-row groups in rotation per wave and fetch a group's next 128-byte line
only for the rows still without a verdict (needle_scan.h, the two-slot loop).  Parity against the CPU oracle on rows built
so that the deciding char sits on either side of every line boundary, in both positions of NEEDLE_PACK_SKIP, on the whole
chip and on 16 CUs (NEEDLE_RESERVE_CUS: 256 waves, so that 60 000 rows already give every wave several groups to rotate --
on the whole chip only batches beyond 524 288 rows reach a wave's second slot).  find() in packed mode runs on the same
batches: its kernel is not part of the change and must answer as before.

One non-GPU test pins the share of the C2 batch's lines that the result needs (the C2 traffic target)."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CODE = r'''
import sys, numpy as np, torch
sys.path.insert(0, "."); sys.path.insert(0, "tests")
from needle_amd import workload as W
from needle_amd.pattern import DFACompiler, unpack_bitmap
from test_compile_matches_txt import oracle_for
small = sys.argv[1] == "small"   # 16 CUs: skip the batches that only make sense on the whole chip

def h32(x):
    return W._hash32(np.asarray(x, dtype=np.int64))

def compiled(rx):
    p = DFACompiler.compile(rx, "t", 0)
    km = p.info()["kernel_mode"]
    assert km["matches"] == 0 and km["contained_in"] == 0 and km["forwards"] == 0, km   # packed functions
    return p, oracle_for(rx, 0)[0]

def positions(n, width, line, kind):
    """Per row the position of its deciding token (-1: nowhere).  `line` = chars per 128-byte line.  kind: "mix" = a layout per
    64-row group, drawn by a hash of the group: all rows early (first line) | exactly one row late | only the 8 rows of one
    load instruction late | no row early | every row on its own | no row with a token; "alt<k>" = blocks of k groups
    all-early / none-early in turn (k = the waves of the launch: a wave's successive groups, and so its two slots, alternate)."""
    r = np.arange(n, dtype=np.int64)
    g, ri = r >> 6, r & 63
    early_set = np.array([0, line - 2, line - 1], dtype=np.int64)
    late_list = [line, line + 1, width - 1, -1]
    for k in range(2, (width + line - 1) // line):   # rows of several lines: both sides of every later boundary
        late_list += [k * line - 1, k * line]
    late_set = np.array([x for x in late_list if x < width], dtype=np.int64)
    hr = h32(r * 2654435761 + 17)
    early = early_set[hr % len(early_set)]
    late = late_set[(hr >> 8) % len(late_set)]
    if width <= line:                                # one chunk: there is no late
        late = early
    if kind.startswith("alt"):
        return np.where((g // int(kind[3:])) % 2 == 0, early, late)
    hg = h32(g * 40503 + 5)
    lay = hg % 6
    one = (hg >> 8) % 64
    instr = (hg >> 16) % 8
    is_late = np.select([lay == 0, lay == 1, lay == 2, lay == 3, lay == 4], [False, ri == one, (ri >> 3) == instr, True, (hr >> 20) % 2 == 1], False)
    pos = np.where(is_late, late, early)
    return np.where(lay == 5, -1, pos)

def build(n, width, dtype, filler, token, pos, tail=None):
    rows = np.full((n, width), filler, dtype=dtype)
    if tail is not None:                             # what lies behind the first line (the "poison")
        rows[:, -len(tail):] = np.asarray(tail, dtype=dtype)
    has = pos >= 0
    for k, t in enumerate(token):
        ok = has & (pos + k < width)
        rows[np.nonzero(ok)[0], pos[ok] + k] = t
    return rows

def ragged(n, width, line):
    pick = np.array([0, 1, line - 1, line, line + 1, width], dtype=np.int64)
    hr = h32(np.arange(n, dtype=np.int64) * 69069 + 3)
    l = np.where(hr % 3 == 0, (hr >> 8) % (width + 1), pick[(hr >> 8) % len(pick)])
    return np.minimum(l, width).astype(np.uint32)

def check(p, o, host, line, tag):
    n, width = host.shape
    dev = torch.from_numpy(host if host.dtype == np.uint8 else host.view(np.int16)).cuda()
    for lens in (None, ragged(n, width, line)):
        tl = None if lens is None else torch.from_numpy(lens.astype(np.int32)).cuda()
        what = tag + (n, width, lens is None)
        assert (unpack_bitmap(p.contained_in_batch(dev, tl), n) == o.batch_contained_in(host, lens, threads=8)).all(), ("containedIn",) + what
        assert (unpack_bitmap(p.matches_batch(dev, tl), n) == o.batch_matches(host, lens, threads=8)).all(), ("matches",) + what
        fw, fs, fe = p.find_batch(dev, tl)
        of, ofs, ofe = o.batch_find(host, lens, threads=8)
        assert (unpack_bitmap(fw, n) == of).all() and (fs.cpu().numpy() == ofs).all() and (fe.cpu().numpy() == ofe).all(), ("find",) + what

# (filler, token): the token decides containedIn() ("accept") or matches() ("kill") where it stands
D = compiled("[0-9]+")
S = compiled("[a-z]+[0-9]")                          # matches(): a sink that rows reach at their first bad char
U = compiled(W.script_regex())                       # C5: a run of >= 3 chars of 42 BMP ranges, UTF-16 rows
a, d5, sp = ord("a"), ord("5"), ord(" ")
CASES = [
    ("D", D, np.uint8, [(a, [d5]), (d5, [a]), (sp, [d5, d5, d5])]),
    ("S", S, np.uint8, [(a, [d5]), (a, [sp]), (sp, [a, d5])]),
    ("U", U, np.uint16, [(0x2000, [0x0391, 0x0392, 0x0393]), (0x0391, [0x2000]), (a, [0x3041, 0x3042, 0x3043, 0x3044])]),
]
counts_full = [1, 63, 64, 65, 16383, 16385, 32769, 60000] + ([] if small else [262143, 262145])
for name, (p, o), dtype, pairs in CASES:
    cw = np.dtype(dtype).itemsize
    line = 128 // cw
    for pi, (filler, token) in enumerate(pairs):
        # row counts at two lines per row; the first pair of the first pattern takes all of them
        for n in (counts_full if (name == "D" and pi == 0) else [65, 16385, 60000]):
            width = 256 // cw
            check(p, o, build(n, width, dtype, filler, token, positions(n, width, line, "mix")), line, (name, pi, "mix"))
        for wb in (128, 192, 384, 1024):             # row widths in bytes: one chunk, a stride that is no multiple of the tile, 3 and 8 lines
            width = wb // cw
            check(p, o, build(60000 if wb < 1024 else 20000, width, dtype, filler, token, positions(60000 if wb < 1024 else 20000, width, line, "mix")), line, (name, pi, "mix"))
    filler, token = pairs[0]
    for k in (256, 4096):                            # all-early / none-early groups in turn along a wave's sequence (16 CUs | the whole chip)
        n = 64 * k * 4 + 64 * 7 + 5
        if small and k == 4096:
            continue
        width = 256 // cw
        check(p, o, build(n, width, dtype, filler, token, positions(n, width, line, "alt%d" % k)), line, (name, "alt", k))

# tail poison: the skipped lines hold what would flip the verdict if they were walked from the start state
n, width = 60000, 256
pos = positions(n, width, 128, "mix")
# containedIn() "yes" in the first line, bytes beyond maxChar (the OVER column) behind
check(D[0], D[1], build(n, width, np.uint8, a, [d5], np.where(pos >= 0, pos % 128, 0), tail=[0xFF] * 100 + [0x80] * 28), 128, ("D", "over-tail", 0))
check(S[0], S[1], build(n, width, np.uint8, a, [d5], np.where(pos >= 0, 1 + pos % 127, 1), tail=[0xFF] * 128), 128, ("S", "over-tail", 0))
# matches() dead in the first line, a full match behind
check(S[0], S[1], build(n, width, np.uint8, a, [sp], pos, tail=[a] * 127 + [d5]), 128, ("S", "match-tail", 0))
check(D[0], D[1], build(n, width, np.uint8, d5, [a], pos, tail=[d5] * 128), 128, ("D", "match-tail", 0))
n, width = 20000, 512
posu = positions(n, width, 64, "mix")
check(U[0], U[1], build(n, width, np.uint16, 0x0391, [0x2000], posu, tail=[0x0391] * 64), 64, ("U", "match-tail", 0))
check(U[0], U[1], build(n, width, np.uint16, 0x2000, [0x0391] * 3, np.where(posu >= 0, posu % 60, 0), tail=[0xFFFE] * 300), 64, ("U", "over-tail", 0))
print("LINE-SKIP-OK")
'''


@pytest.mark.gpu
@pytest.mark.parametrize("cus", ["chip", "small"])
@pytest.mark.parametrize("skip", [None, "0"])
def test_two_slot_scan_matches_oracle(skip, cus):
    env = dict(os.environ)
    env.pop("NEEDLE_PACK_SKIP", None)
    if skip is not None:
        env["NEEDLE_PACK_SKIP"] = skip
    if cus == "small":
        env["NEEDLE_RESERVE_CUS"] = "240"
    r = subprocess.run([sys.executable, "-c", CODE, cus], env=env, capture_output=True, text=True, timeout=1500, cwd=ROOT)
    assert "LINE-SKIP-OK" in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]


def test_c2_needed_lines_fraction():
    """The C2 batch (bench.py: digits_batch rows 0 .. 10^7 - 1, 256 bytes = two 128-byte lines each): containedIn() of `[0-9]+`
    is decided at a row's first digit, so the second line of a row whose digit run starts in chars 0 .. 127 is not needed.
    Recomputed from the generator's row hash: needed lines / all lines = 0.8737."""
    from needle_amd import workload as W
    n, n_cols = 10_000_000, 256
    r = np.arange(n, dtype=np.int64)
    h = W._hash32((W.SEED ^ 0x9E3779B9) + r * 40503)
    plant = (h & 1) == 1
    run = 1 + ((h >> 1) % 6)
    pos = (h >> 8) % (n_cols - run + 1)
    early = int((plant & (pos < 128)).sum())
    # (the generator itself on a sample: the planted run is where the hash says, and nothing else in a row is a digit)
    sample = W.digits_batch(np, 0, 4096, n_cols)
    is_digit = (sample >= 48) & (sample <= 57)
    first = np.where(is_digit.any(axis=1), is_digit.argmax(axis=1), -1)
    assert (first == np.where(plant[:4096], pos[:4096], -1)).all()
    assert abs(early / n - 0.2525) < 0.0002
    assert abs((2 * n - early) / (2 * n) - 0.8737) < 0.0001
