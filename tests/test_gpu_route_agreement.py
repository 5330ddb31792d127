"""The two row layouts agree on the route (choose_route in needle_amd/csrc/needle_api.cpp): a pattern takes the n-gram candidate filter on
PACKED rows exactly when it takes it on the same rows laid out at a FIXED stride -- except where the routing documents a difference
(find() of a pattern without bounded match lengths: behind the filter at a fixed stride only).  `filter_launches` of
needle_pattern_prefilter_state says which kernel ran.

One seeded batch per case: 256 rows of 1 .. 120 chars, padded to a stride of 128 chars for the fixed form (the fixed-stride filter kernel
wants rows at least 64 bytes apart and 16 KiB in all: a smaller batch would skip the filter on that side only).  The prefilter is pinned ON.
Every cell: both layouts' answers equal the CPU oracle's on every row, and the launch counter moved by exactly the expected amount.

What other tests assert already is not repeated: containedIn() / find() / matches() / cursors of the 8-bit dictionary on packed rows under ON
(test_gpu_packed_prefilter.py::test_which_kernel_ran_auto_on_off) -- here that pattern's cells are the fixed-stride ones and the two
layouts side by side."""
import os
import subprocess
import sys

import numpy as np
import pytest

from test_gpu_configs import compiled
from test_gpu_packed_dev import device_packed, oracle_packed

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_ROWS, MAX_LEN, STRIDE = 256, 120, 128
NAMES = ["Sherlock", "Holmes", "Watson", "Moriarty", "Mycroft", "Baskerville"]


def cyr(w):
    return "".join(chr(0x0430 + ord(c) - 97) for c in w)


def launches(p):
    return p.prefilter_state("forwards")["filter_launches"] + p.prefilter_state("contained_in")["filter_launches"]


def batch(words, alphabet, dtype, seed, tails=None):
    """256 rows of 1 .. 120 chars from `alphabet`, a word planted in every other row that can hold it (followed by tails[k], if given)."""
    rng = np.random.default_rng(seed)
    al = np.array([ord(c) for c in alphabet], dtype=dtype)
    rows = []
    for i in range(N_ROWS):
        r = rng.choice(al, int(rng.integers(1, MAX_LEN + 1))).astype(dtype)
        k = int(rng.integers(0, len(words)))
        w = words[k] + (tails[k % len(tails)] if tails else "")
        if i % 2 == 0 and r.size >= len(w):
            at = int(rng.integers(0, r.size - len(w) + 1))
            r[at:at + len(w)] = [ord(c) for c in w]
        rows.append(r)
    return rows


def agree(p, o, rows, dtype, fixed_find, packed_find, fixed_contained=1, packed_contained=1, what=""):
    """containedIn() and find() of `rows` in both layouts under ON: the oracle's answers on every row; the launch counter moves by the
    expected amount per call.  matches() and find() from per-row cursors: the counter stays put on either layout."""
    import torch
    from needle_amd.pattern import unpack_bitmap
    n = len(rows)
    wm, wc, wf, ws, we = oracle_packed(o, rows, dtype)
    assert wf.sum() > 20 and not wf.all(), (what, "the batch does not exercise the pattern", int(wf.sum()))
    host = np.zeros((n, STRIDE), dtype=dtype)
    for i, r in enumerate(rows):
        host[i, :r.size] = r
    fixed = torch.from_numpy(host if dtype == np.uint8 else host.view(np.int16)).cuda()
    lens = torch.tensor([r.size for r in rows], dtype=torch.int32, device="cuda")
    data, offsets = device_packed(rows, dtype, 5, 7, None)
    zero = torch.zeros(n, dtype=torch.int32, device="cuda")
    p.set_prefilter(p.PREFILTER_ON)
    moved = {}

    def cell(name, call):
        before = launches(p)
        out = call()
        torch.cuda.synchronize()
        moved[name] = launches(p) - before
        return out

    fc = cell("fixed containedIn", lambda: p.contained_in_batch(fixed, lens))
    pc = cell("packed containedIn", lambda: p.contained_in_packed(data, offsets))
    ff = cell("fixed find", lambda: p.find_batch(fixed, lens))
    pf = cell("packed find", lambda: p.find_packed(data, offsets))
    fm = cell("fixed matches", lambda: p.matches_batch(fixed, lens))
    pm = cell("packed matches", lambda: p.matches_packed(data, offsets))
    fn = cell("fixed cursors", lambda: p.find_next_batch(fixed, zero, lens))
    pn = cell("packed cursors", lambda: p.find_next_packed(data, offsets, zero))
    p.set_prefilter(p.PREFILTER_AUTO)
    print(what, moved)
    for name, words, want in (("fixed containedIn", fc, wc), ("packed containedIn", pc, wc), ("fixed matches", fm, wm), ("packed matches", pm, wm)):
        assert (unpack_bitmap(words, n) == want).all(), (what, name, "differs from the oracle")
    for name, (w, s, e) in (("fixed find", ff), ("packed find", pf), ("fixed cursors", fn), ("packed cursors", pn)):
        assert (unpack_bitmap(w, n) == wf).all() and (s.cpu().numpy()[:n] == ws).all() and (e.cpu().numpy()[:n] == we).all(), (what, name, "differs from the oracle")
    want_moved = {"fixed containedIn": fixed_contained, "packed containedIn": packed_contained, "fixed find": fixed_find, "packed find": packed_find,
                  "fixed matches": 0, "packed matches": 0, "fixed cursors": 0, "packed cursors": 0}
    assert moved == want_moved, (what, "filter launches per call", moved, "expected", want_moved)


def dictionary():
    from needle_amd import workload as W
    return W.keywords(1000, min_len=6, max_len=8)


@pytest.mark.gpu
def test_dictionary_8bit_lds_program_with_its_own_filter():
    words = dictionary()
    p, o = compiled("|".join(words))
    assert p.info()["kernel_mode"]["forwards"] == 6 and p.prefilter_info("forwards")["on"]
    agree(p, o, batch(words, "abcdefghijklmnopqrstuvwxyz ", np.uint8, 1), np.uint8, fixed_find=1, packed_find=1, what="8-bit dictionary")


@pytest.mark.gpu
def test_dictionary_utf16_page_0():
    words = dictionary()
    p, o = compiled("|".join(words))
    assert p.utf16_route() is not None and p.utf16_route()[0] == 0
    agree(p, o, batch(words, "abcdefghijklmnopqrstuvwxyz 一š", np.uint16, 2), np.uint16, fixed_find=1, packed_find=1, what="UTF-16, page 0")


@pytest.mark.gpu
def test_dictionary_utf16_page_4():
    words = [cyr(w) for w in dictionary()]
    p, o = compiled("|".join(words))
    assert p.utf16_route() is not None and p.utf16_route()[0] == 4
    al = "".join(chr(0x0430 + k) for k in range(26)) + " a一"
    agree(p, o, batch(words, al, np.uint16, 3), np.uint16, fixed_find=1, packed_find=1, what="UTF-16, page 4")


CHILD = r'''
import sys
sys.path.insert(0, "."); sys.path.insert(0, "tests")
import numpy as np
import test_gpu_route_agreement as T
case = sys.argv[1]
if case == "wide":          # NEEDLE_PREFILTER=2: the small two-script automaton takes the WIDE route
    words = T.NAMES + [T.cyr(w.lower()) for w in T.NAMES]
    p, o = T.compiled("|".join(words))
    assert p.utf16_route() is None and p.prefilter_info("forwards", wide=True)["on"]
    al = "SherlockHmsWatnMiyfBv " + "".join(sorted(set("".join(words[6:]))))
    T.agree(p, o, T.batch(words, al, np.uint16, 4), np.uint16, fixed_find=1, packed_find=1, what="UTF-16, two scripts (WIDE)")
elif case == "hbm":         # NEEDLE_MAX_PROG_LDS lowered: the ordinary program is a hot-rows / HBM-table one, the filter program walks out of HBM / L2
    words = T.dictionary()
    p, o = T.compiled("|".join(words))
    assert p.info()["kernel_mode"]["forwards"] in (3, 5) and p.prefilter_info("forwards")["on"]
    T.agree(p, o, T.batch(words, "abcdefghijklmnopqrstuvwxyz ", np.uint8, 5), np.uint8, fixed_find=1, packed_find=1, what="8-bit dictionary, HBM-table filter program")
elif case == "unbounded":   # NEEDLE_PREFILTER=2: find() without bounded match lengths -- behind the filter at a fixed stride only (the documented difference)
    p, o = T.compiled("(" + "|".join(T.NAMES) + ")[0-9]+")
    assert p.prefilter_info("forwards")["on"] and p.prefilter_info("contained_in")["on"]
    T.agree(p, o, T.batch(T.NAMES, "SherlockHmsWatnMiyfBv 0123456789", np.uint8, 6, tails=["1", "22", "333"]), np.uint8, fixed_find=1, packed_find=0,
            what="(names)[0-9]+")
print("ROUTE-CHILD-OK")
'''


@pytest.mark.gpu
@pytest.mark.parametrize("case,env", [("wide", {"NEEDLE_PREFILTER": "2"}), ("hbm", {"NEEDLE_MAX_PROG_LDS": "4096", "NEEDLE_SPARSE": "0"}),
                                      ("unbounded", {"NEEDLE_PREFILTER": "2", "NEEDLE_PAIR_MAX_BYTES": "0"})])
def test_routes_that_need_a_switch(case, env):
    """(the switches are read once per process: a child)"""
    r = subprocess.run([sys.executable, "-c", CHILD, case], env=dict(os.environ, **env), capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert "ROUTE-CHILD-OK" in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]
