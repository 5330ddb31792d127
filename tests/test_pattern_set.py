"""Pattern sets on the CPU (needle_pattern_set_*, needle_set_*_packed_*; needle_amd/csrc/needle_set.cpp): the ABI and its argument checks
without a device, the product automata (PatternSet.tables()) walked in Python against the oracle per pattern, the state counts of the
accept-OR construction, the grouping, and the refusal of a big dictionary."""
import ctypes
import os
import random
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT
from pattern_set_cases import (BIG, OLDER_GPU_SETS, OPS_WIDTHS, PLANS, SETS, TABLE8, alphabet_and_pieces, assert_plan, compile_set, fuzz_alphabet,
                               fuzz_counters, ladder_shape, oracle_masks, random_set, split_case, units, walk_tables)

NAMES = ["needle_pattern_set_create", "needle_pattern_set_destroy", "needle_pattern_set_info", "needle_pattern_set_get_tables",
         "needle_set_matches_packed_dev", "needle_set_contained_in_packed_dev", "needle_set_matches_packed_host",
         "needle_set_contained_in_packed_host"]


@pytest.fixture(scope="module")
def lib():
    from needle_amd import build
    build.build()
    from oracle import walker
    walker.build()
    from needle_amd import _lib
    return _lib.lib()


def test_symbols_are_exported(lib):
    from needle_amd import _lib
    for n in NAMES:
        assert hasattr(lib, n) and n in _lib.EXPORTS, n


def test_argument_checks_need_no_device(lib):
    from needle_amd import _lib
    from needle_amd.pattern import DFACompiler, PatternSet
    ps = PatternSet([DFACompiler.compile("[0-9]+", "d"), DFACompiler.compile("ab", "e")])
    data = np.frombuffer(b"ab12cd..", dtype=np.uint8).copy()
    offsets = np.array([0, 4, 6], dtype=np.uint64)
    masks = np.zeros(2, dtype=np.uint32)

    def view(data_ptr=data.ctypes.data, cw=1, n=2, off=offsets.ctypes.data):
        v = _lib.PackedView()
        v.data, v.char_width, v.n_rows, v.offsets = data_ptr, cw, n, off
        return v
    for fn in (lib.needle_set_matches_packed_dev, lib.needle_set_contained_in_packed_dev):
        assert fn(None, ctypes.byref(view()), masks.ctypes.data, None) == _lib.ERR_INVALID          # NULL set
        assert fn(ps._h, None, masks.ctypes.data, None) == _lib.ERR_INVALID                         # NULL view
        assert fn(ps._h, ctypes.byref(view(off=None)), masks.ctypes.data, None) == _lib.ERR_INVALID # NULL offsets
        assert fn(ps._h, ctypes.byref(view()), None, None) == _lib.ERR_INVALID                      # NULL masks
        assert fn(ps._h, ctypes.byref(view(cw=3)), masks.ctypes.data, None) == _lib.ERR_INVALID     # bad char_width
        assert fn(ps._h, ctypes.byref(view(data_ptr=data.ctypes.data + 1)), masks.ctypes.data, None) == _lib.ERR_INVALID  # not 4-byte aligned
        assert fn(ps._h, ctypes.byref(view(n=0)), masks.ctypes.data, None) == _lib.NEEDLE_OK        # an empty batch
    for fn in (lib.needle_set_matches_packed_host, lib.needle_set_contained_in_packed_host):
        assert fn(None, ctypes.byref(view()), masks.ctypes.data) == _lib.ERR_INVALID
        assert fn(ps._h, ctypes.byref(view(cw=0)), masks.ctypes.data) == _lib.ERR_INVALID
        assert fn(ps._h, ctypes.byref(view()), None) == _lib.ERR_INVALID
        assert fn(ps._h, ctypes.byref(view(n=0)), masks.ctypes.data) == _lib.NEEDLE_OK
    assert ps.contained_in_packed(np.zeros(0, dtype=np.uint8), np.zeros(1, dtype=np.uint64)).size == 0
    info = _lib.SetInfo()
    assert lib.needle_pattern_set_info(ps._h, 2, 1, ctypes.byref(info)) == _lib.ERR_INVALID
    assert lib.needle_pattern_set_info(ps._h, 0, 3, ctypes.byref(info)) == _lib.ERR_INVALID
    assert lib.needle_pattern_set_get_tables(ps._h, 0, 1, 5, None, None, None, None, None, 0, None, 0) == _lib.ERR_INVALID


def test_create_refuses_bad_sets(lib):
    from needle_amd import _lib
    from needle_amd.pattern import DFACompiler, PatternSet
    p = DFACompiler.compile("ab", "p")
    with pytest.raises(ValueError):
        PatternSet([p] * 33)
    with pytest.raises(ValueError):
        PatternSet([])
    assert PatternSet([p] * 32).info()["n_patterns"] == 32
    arr = (ctypes.c_void_p * 2)(p._h, None)  # a NULL member
    h = ctypes.c_void_p()
    assert lib.needle_pattern_set_create(arr, 2, ctypes.byref(h)) == _lib.ERR_INVALID and not h.value


def test_set_outlives_its_patterns(lib):
    from needle_amd.pattern import DFACompiler, PatternSet
    pats = [DFACompiler.compile(x, "p") for x in ("[0-9]+", "ab")]
    ps = PatternSet(pats)
    del pats
    t = ps.tables("contained_in", 1, 0)
    assert [walk_tables(t, units(x, np.uint8), "contained_in") for x in ("xx7ab", "ab", "7", "x")] == [3, 2, 1, 0]
    t = ps.tables("matches", 1, 0)
    assert [walk_tables(t, units(x, np.uint8), "matches") for x in ("xx7ab", "ab", "7", "x")] == [0, 2, 1, 0]


def seeded_rows(name, n, seed, dtype=None):
    alphabet, pieces = alphabet_and_pieces(name, dtype)
    dtype = SETS[name][1] if dtype is None else dtype
    rng = random.Random(seed)
    rows = []
    for i in range(n):
        k = rng.randrange(0, 41)
        text = [rng.choice(alphabet) for _ in range(k)]
        mode = rng.random()
        if mode < 0.15:    # exactly one piece: a whole-row match
            text = list(rng.choice(pieces))
        elif mode < 0.6:   # one or two pieces somewhere
            for _ in range(rng.randrange(1, 3)):
                at = rng.randrange(0, len(text) + 1)
                text[at:at] = list(rng.choice(pieces))
        rows.append(units("".join(text), dtype))
    rows[0] = units("", dtype)
    return rows


NEW_SETS = ["edge255", "edge256", "count260", "count260ci", "tail5"]


@pytest.mark.parametrize("case", ["nullable4", "logs8", "kw32", "mix16", "u16b"] + [s + w for s in NEW_SETS for w in ("@8", "@16")])
def test_tables_walked_in_python_equal_the_oracle(lib, case):
    name, dtype = split_case(case)
    ps, oracles, dtype = compile_set(name, dtype)
    k = len(oracles)
    rows = seeded_rows(name, 2000, 1234, dtype)
    want_m, want_c = oracle_masks(oracles, rows, dtype)
    assert all(((want_c >> i) & 1).sum() >= 3 for i in range(k)), "every pattern is found in some rows"
    cw = np.dtype(dtype).itemsize
    for op, want in (("matches", want_m), ("contained_in", want_c)):
        info = ps.info(op, cw)
        assert info["n_patterns"] == k
        got = np.zeros(len(rows), np.uint32)
        nxt = 0
        for g, gi in enumerate(info["groups"]):
            assert gi["first_pattern"] == nxt and gi["pattern_count"] >= 1  # the groups partition 0 .. k-1 in order
            nxt += gi["pattern_count"]
            t = ps.tables(op, cw, g)
            assert (gi["n_states"], gi["n_columns"]) == (t["n_states"], t["n_classes"] + 2)  # info() agrees with tables()
            assert t["table"].shape == (t["n_states"], t["n_classes"]) and int(t["class_map"].max()) == t["n_classes"] - 1
            group_bits = ((1 << gi["pattern_count"]) - 1) << gi["first_pattern"]
            assert not (int(np.bitwise_or.reduce(t["masks"])) & ~group_bits)
            got |= np.array([walk_tables(t, r, op) for r in rows], dtype=np.uint32)
        assert nxt == k
        bad = np.nonzero(got != want)[0]
        assert bad.size == 0, (name, op, bad[:5], [bytes(rows[i]) for i in bad[:3]], got[bad[:5]], want[bad[:5]])
        assert not (got >> np.uint32(k)).any() if k < 32 else True


def test_kernel_modes_of_the_named_sets(lib):
    """n_states, kernel_mode and lds_bytes of every (set, op, char width) a GPU test launches."""
    # Why it matters: these numbers decide which instantiations of packed_set_kernel (op x width x element size x window bytes) and of
    # set_spans_kernel (width x element size) each GPU test reaches.  The older sets are all 8-bit tables with 128-byte windows; the
    # 16-bit tables, the 64-byte windows (lds_bytes > 65536) and the boundary between the element sizes are reached by PLANS' sets only.
    for name in PLANS:
        ps, _, _ = compile_set(name)
        for op, cw in OPS_WIDTHS:
            g = assert_plan(name, ps, op, cw)
            waves, chb = ladder_shape(g["lds_bytes"])
            assert (waves, chb) == ((16, 64) if g["lds_bytes"] > 65536 else (16, 128)), (name, op, cw, g)
    big = [(n, op, cw) for n in PLANS for op, cw in OPS_WIDTHS if PLANS[n][2][OPS_WIDTHS.index((op, cw))] == BIG]
    assert big == [("tail5", "matches", 1), ("tail5", "matches", 2), ("mix16", "contained_in", 1), ("mix16", "contained_in", 2)]
    # edge255: the largest program with 8-bit elements (device states are the product's + 1: 0 is the sink, the highest is 255)
    ps, _, _ = compile_set("edge255")
    assert all(ps.tables(op, cw, 0)["n_states"] + 1 == 256 for op, cw in OPS_WIDTHS)
    for name in OLDER_GPU_SETS:
        ps, _, dtype = compile_set(name)
        for op, cw in OPS_WIDTHS:
            if cw == 1 and dtype == np.uint16:  # (the older UTF-16 set runs on UTF-16 rows only)
                continue
            for g in ps.info(op, cw)["groups"]:
                assert g["kernel_mode"] == TABLE8 and g["lds_bytes"] <= 32768 and ladder_shape(g["lds_bytes"]) == (16, 128), (name, op, cw, g)


FUZZ_SEEDS = range(6)   # chosen so that the conditions of test_random_sets_reach_both_table_widths_and_several_groups hold
FUZZ_SETS_PER_SEED = 20
_fuzz = {}


def fuzz_seed(seed):
    """The sets of one seed walked against the oracle, once per process -> (drawn, skipped, TABLE16 plans, sets cut into groups)."""
    if seed in _fuzz:
        return _fuzz[seed]
    rng = random.Random(7000 + seed)
    nrng = np.random.default_rng(seed)
    rows = {cw: [nrng.choice(fuzz_alphabet(dt), int(n)).astype(dt) for n in nrng.integers(0, 24, 300)] for cw, dt in ((1, np.uint8), (2, np.uint16))}
    skipped = table16 = grouped = 0
    for _ in range(FUZZ_SETS_PER_SEED):
        members, ps, oracles, infos = random_set(rng)
        if ps is None:
            skipped += 1
            continue
        t16, grp = fuzz_counters(infos)
        table16, grouped = table16 + t16, grouped + grp
        want = {cw: oracle_masks(oracles, rows[cw], rows[cw][0].dtype) for cw in (1, 2)}
        for op, cw in OPS_WIDTHS:
            got = np.zeros(len(rows[cw]), np.uint32)
            for g in range(infos[op, cw]["n_groups"]):
                t = ps.tables(op, cw, g)
                got |= np.array([walk_tables(t, r, op) for r in rows[cw]], dtype=np.uint32)
            bad = np.nonzero(got != want[cw][op == "contained_in"])[0]
            assert bad.size == 0, (seed, members, op, cw, [rows[cw][i].tolist() for i in bad[:3]], got[bad[:3]], want[cw][op == "contained_in"][bad[:3]])
    _fuzz[seed] = (FUZZ_SETS_PER_SEED, skipped, table16, grouped)
    return _fuzz[seed]


@pytest.mark.parametrize("seed", FUZZ_SEEDS)
def test_random_sets_walked_in_python_equal_the_oracle(lib, seed):
    """Sets of 1 .. 32 random regexes x random flag sets (pattern_set_cases.random_set): every group's product walked in Python, OR-ed,
    against the members' own oracles -- both ops, both char widths, 300 rows of 0 .. 23 chars of the fuzz alphabet and the fold partners."""
    print("seed %d: drawn %d, skipped %d, TABLE16 plans %d, grouped sets %d" % ((seed,) + fuzz_seed(seed)))


def test_random_sets_reach_both_table_widths_and_several_groups(lib):
    """Over all seeds (walked here when their own tests were not): at least 10 plans with 16-bit elements, at least one set cut into
    several groups, at most 5 % of the drawn sets refused by PatternSet(...) or info()."""
    drawn, skipped, table16, grouped = (sum(x) for x in zip(*[fuzz_seed(s) for s in FUZZ_SEEDS]))
    print("random sets: drawn %d, skipped %d, TABLE16 plans %d, grouped sets %d" % (drawn, skipped, table16, grouped))
    assert table16 >= 10 and grouped >= 1 and skipped * 20 <= drawn, (drawn, skipped, table16, grouped)


def test_state_counts_are_of_the_accept_or_order(lib):
    """Keeping "which patterns have matched so far" in the state needs 5944 states for logs8 and grows as 2^k; the accept-OR product has 145."""
    ps, _, _ = compile_set("logs8")
    for cw in (1, 2):
        i = ps.info("contained_in", cw)
        assert i["n_groups"] == 1 and i["groups"][0]["n_states"] < 1000 and i["groups"][0]["pattern_count"] == 8
        assert ps.info("matches", cw)["n_groups"] == 1 and ps.info("matches", cw)["groups"][0]["n_states"] < 200
    ps, _, _ = compile_set("kw32")
    for op in ("matches", "contained_in"):
        i = ps.info(op, 1)
        assert i["n_groups"] == 1 and i["groups"][0]["pattern_count"] == 32 and i["groups"][0]["kernel_mode"] in (1, 2)


def test_a_lower_budget_cuts_the_set_into_groups_in_order():
    """NEEDLE_MAX_PROG_LDS below logs8's one product: several groups, consecutive, covering 0 .. 7, each within the budget."""
    code = ("import sys; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
            "from pattern_set_cases import compile_set\n"
            "ps, _, _ = compile_set('logs8')\n"
            "for op in ('matches', 'contained_in'):\n"
            "    i = ps.info(op, 1)\n"
            "    nxt = 0\n"
            "    for g in i['groups']:\n"
            "        assert g['first_pattern'] == nxt and g['lds_bytes'] <= 4096, g\n"
            "        nxt += g['pattern_count']\n"
            "    assert nxt == 8 and i['n_groups'] >= 2, i\n"
            "print('OK')\n" % (ROOT, os.path.join(ROOT, "tests")))
    out = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, NEEDLE_MAX_PROG_LDS="4096"), capture_output=True, text=True)
    assert out.returncode == 0 and "OK" in out.stdout, out.stderr[-2000:]


def test_a_big_dictionary_member_is_refused_by_index(lib):
    from needle_amd import workload as W
    from needle_amd.pattern import DFACompiler, PatternClassCompilationException, PatternSet
    small = DFACompiler.compile("[0-9]+", "d")
    big = DFACompiler.compile("|".join(W.keywords(3000)), "big")
    with pytest.raises(PatternClassCompilationException, match=r"pattern 2 of the set"):
        PatternSet([small, small, big, small])


def test_an_8bit_product_tells_only_the_chars_below_256_apart(lib):
    """Members that differ only above 255 share their 8-bit columns and states: the product for char_width 1 is that of one member, the
    one for char_width 2 tells them apart."""
    from needle_amd.pattern import DFACompiler, PatternSet
    one = PatternSet([DFACompiler.compile("a[b-d]+", "p")])
    two = PatternSet([DFACompiler.compile("a[b-d]+", "p"), DFACompiler.compile("a[b-dα-ω]+", "q")])
    for op in ("matches", "contained_in"):
        g1, g2 = one.info(op, 1)["groups"][0], two.info(op, 1)["groups"][0]
        assert (g2["n_states"], g2["n_columns"]) == (g1["n_states"], g1["n_columns"]) and g2["pattern_count"] == 2
        assert two.info(op, 2)["groups"][0]["n_columns"] > g2["n_columns"]
        assert not two.tables(op, 1, 0)["class_map"][256:].any()
        t = two.tables(op, 2, 0)
        assert [walk_tables(t, units(x, np.uint16), op) for x in ("abc", "aβ", "aa")] == [3, 2, 0]
        t = two.tables(op, 1, 0)
        assert [walk_tables(t, units(x, np.uint8), op) for x in ("abc", "ab", "aa")] == [3, 3, 0]


def test_a_member_the_utf16_column_maps_refuse_leaves_the_set_to_8bit_rows(lib):
    """UTF-16 column offsets are bytes (columns x element size <= 255): 128 classes with more than 255 states fit the 8-bit map only.
    The set is created; char_width 2 is refused where it is asked for, naming the pattern."""
    from needle_amd import _lib
    from needle_amd.pattern import DFACompiler, PatternClassCompilationException, PatternSet
    chars = "".join(chr(c) for c in list(range(0x30, 0x3A)) + list(range(0x41, 0x5B)) + list(range(0x61, 0x7B)) + list(range(0xC0, 0x100)))
    chars += "_ "
    assert len(set(chars)) == 128
    word = chars + chars  # 256 chars: 257 states and the sink
    ps = PatternSet([DFACompiler.compile("ab", "s"), DFACompiler.compile(word, "w")])
    for op in ("matches", "contained_in"):
        i = ps.info(op, 1)
        assert sum(g["pattern_count"] for g in i["groups"]) == 2
        got = 0
        for g in range(i["n_groups"]):
            got |= walk_tables(ps.tables(op, 1, g), units(word, np.uint8), op)
        assert got == (2 if op == "matches" else 3)  # ("ab" is a piece of the word)
        with pytest.raises(PatternClassCompilationException, match=r"pattern 1 of the set.*char_width 2"):
            ps.info(op, 2)
        with pytest.raises(PatternClassCompilationException, match=r"pattern 1 of the set"):
            ps.tables(op, 2, 0)
    data, offsets, masks = np.zeros(4, np.uint16), np.array([0, 2, 4], dtype=np.uint64), np.zeros(2, np.uint32)
    v = _lib.PackedView()
    v.data, v.char_width, v.n_rows, v.offsets = data.ctypes.data, 2, 2, offsets.ctypes.data
    assert lib.needle_set_matches_packed_host(ps._h, ctypes.byref(v), masks.ctypes.data) == _lib.ERR_UNSUPPORTED
    assert lib.needle_set_contained_in_packed_dev(ps._h, ctypes.byref(v), masks.ctypes.data, None) == _lib.ERR_UNSUPPORTED
