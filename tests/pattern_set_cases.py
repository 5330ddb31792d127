"""The pattern sets of the PatternSet tests (test_pattern_set.py on the CPU, test_gpu_pattern_set.py on the GPU): patterns, alphabets,
planted pieces, and the reference answers -- per pattern, by the oracle walking each member's own tables."""
import numpy as np

LOGS8 = ["[0-9]+", "ERROR|WARN|FATAL", "http://.+", r"[a-z]+@[a-z]+\.com", "Sherlock|Holmes|Watson|Irene|Adler|John|Baker",
         "timeout after [0-9]+ms", "(ab|a|bcdef|g)+", "a.c"]
LOGS8_ALPHABET = "hijklmnopqrstuvwxyz _-"
LOGS8_PIECES = ["42", "ERROR", "http://x", "joe@site.com", "Holmes", "timeout after 12ms", "abg", "a-c", "FATAL", "Baker"]
KW32 = ("error warning fatal timeout refused denied panic abort crash failed invalid missing corrupt overflow deadlock retry expired "
        "killed oom segfault leak stall reset dropped blocked unknown illegal broken hang fault lost alarm").split()
assert len(set(KW32)) == 32 and all(3 <= len(w) <= 9 for w in KW32)

SETS = {
    # name: (patterns, numpy dtype of the rows, alphabet, pieces)
    "nullable4": (["[a-c]*", "x|yz", "[0-9]+", "a.c"], np.uint8, "abcxyz019 .-", ["abc", "x", "yz", "123", "a-c", "cab", "7"]),
    "logs8": (LOGS8, np.uint8, LOGS8_ALPHABET, LOGS8_PIECES),
    "mix16": (LOGS8 + ["[A-Z][a-z]+ [A-Z][a-z]+", r"[0-9]+\.[0-9]+\.[0-9]+\.[0-9]+", "user=[a-z]+", "(GET|POST|PUT) /", "0x[0-9a-f]+",
                       r"[a-z]+\.(png|jpg|gif)", "error.*disk", r"\[[0-9]+\]"], np.uint8, LOGS8_ALPHABET + "=.[]",
              LOGS8_PIECES + ["John Smith", "10.0.0.1", "user=bob", "GET /", "0x1f", "cat.png", "error on disk", "[42]"]),
    "kw32": (KW32, np.uint8, "abcdefghijklmnopqrstuvwxyz ", KW32),
    "u16b": (["[α-ω]+", "ε|λ", "[Ѐ-ӿ]+х", "ab", "[一-龥]{2}"], np.uint16, "cdxyz ́あ￿", ["αβγ", "ε", "λ", "жх", "ab", "一二"]),
}

# The sets below exist for the kernel instantiations the ones above never reach (test_pattern_set.test_kernel_modes_of_the_named_sets
# asserts their sizes): products of more than 255 states (16-bit table elements), programs above 64 KB (64-byte windows), the
# boundary between the two element widths, and members compiled with flags.  An entry may carry a fifth value: the flags common to
# its members (set_flags).
CASE_INSENSITIVE, UNICODE_CASE, DOTALL = 0x02, 0x40, 0x20  # (needle_amd.pattern's values; compile_set checks them)
RUN260 = ("efg" * 87)[:260]  # [e-g]{260}


def edge_pieces(k):
    """Whole rows around a{k}: k `a`s first (the one that matches: its three whole-row turns come first), the runs of 0, 1 and
    253 .. 257 `a`s, and a 254- and a k-run with a `b` behind and in front (containedIn only)."""
    runs = ["a" * k] + ["a" * n for n in (0, 1, 253, 254, 255, 256, 257) if n != k]
    tails = ["a" * k + "b", "b" + "a" * k] + (["a" * 254 + "b", "b" + "a" * 254] if k != 254 else [])
    return runs + tails


COUNT260 = ["[e-g]{260}x", "[b-d]{2,5}y", "[0-9]+", "ab"]
COUNT260_PIECES = [RUN260 + "x", "bcdy", "42", "ab", RUN260[:259] + "x", "g" + RUN260 + "x", "bbbbby", "7"]
SETS.update({
    "edge255": (["a{254}"], np.uint8, "aab", edge_pieces(254)),   # 255 states: the last program with 8-bit elements, device states 0 .. 255
    "edge256": (["a{255}"], np.uint8, "aab", edge_pieces(255)),   # 256 states: the first one with 16-bit elements
    "count260": (COUNT260, np.uint8, "efgbcdxya019 _", COUNT260_PIECES),
    # (the fold partners: U+212A KELVIN SIGN ~ k, U+00B5 MICRO SIGN ~ U+03BC ~ U+039C; U+0130 and U+017F fold to i and s)
    "count260ci": (COUNT260 + ["kelvin|µm", "[α-ω]{2,40}"], np.uint16,
                   "efgbcdxya019 _EFGBkK\u212a\u00b5\u03bc\u0130\u017f\uffffαΩ",
                   COUNT260_PIECES[:4] + [RUN260.upper() + "X", RUN260[:130] + RUN260[130:].upper() + "X", "KELVIN", "ΑΒΓ",
                                          "\u212aelvin", "\u03bcm", "\u039cm", "\u00b5m", "BcDy", "aB", "\u00b5\u00b5\u00b5", "kelvin",
                                          "βΩ"],
                   CASE_INSENSITIVE | UNICODE_CASE),
    "tail5": ([".*[ab].{5}", ".*[bc].{5}", ".*[ca].{5}", "[0-9]+"], np.uint8, "abcxyz019\n ", ["a12345", "b\n\n\n\n\n", "xxc01234", "42", "7", "123456"],
              DOTALL),
})
# What gpu_batch is given beyond its defaults, per set: rows long enough to hold a 261-char match inside them, and a whole-row piece
# every third row where a set has more pieces than the 27 rows of the default recipe give three turns each.
GPU_RECIPE = {"count260": dict(lengths="long"), "count260ci": dict(lengths="long", piece_every=3), "mix16": dict(piece_every=3)}


def set_flags(name):
    return SETS[name][4] if len(SETS[name]) > 4 else 0


def split_case(case):
    """"name" -> (name, the set's own dtype); "name@8" / "name@16" -> the set on 8-bit / UTF-16 rows."""
    name, _, bits = case.partition("@")
    return name, {"": SETS[name][1], "8": np.uint8, "16": np.uint16}[bits]


def alphabet_and_pieces(name, dtype=None):
    """A set's alphabet and pieces for rows of `dtype` (default: the set's own).  8-bit rows keep the chars below 256 and the pieces
    made of them; UTF-16 rows of a set written for 8-bit rows get chars whose LOW byte is a char of the alphabet (a kernel that drops
    the high byte reads them as that char) and U+FFFF."""
    own, alphabet, pieces = SETS[name][1:4]
    if dtype is None or np.dtype(dtype) == np.dtype(own):
        return alphabet, pieces
    if np.dtype(dtype) == np.uint8:
        return "".join(c for c in alphabet if ord(c) < 256), [p for p in pieces if all(ord(c) < 256 for c in p)]
    return alphabet + "".join(chr(0x100 | ord(c)) for c in alphabet[:3]) + "￿", pieces


def units(text, dtype):
    return np.array([ord(ch) for ch in text], dtype=dtype)


def compile_set(name, dtype=None):
    """(PatternSet, [per-pattern oracle], dtype) of a set above, its members compiled with the set's flags; dtype: the rows' (default:
    the set's own)."""
    from needle_amd import pattern as P
    from test_compile_matches_txt import oracle_for
    assert (CASE_INSENSITIVE, UNICODE_CASE, DOTALL) == (P.CASE_INSENSITIVE, P.UNICODE_CASE, P.DOTALL)
    pats, flags = SETS[name][0], set_flags(name)
    return (P.PatternSet([P.DFACompiler.compile(p, "p%d" % i, flags) for i, p in enumerate(pats)]), [oracle_for(p, flags)[0] for p in pats],
            SETS[name][1] if dtype is None else dtype)


def oracle_masks(oracles, rows, dtype):
    """(matches masks, containedIn masks) uint32[n] of the rows: bit i = what pattern i's oracle answers; rows bucketed by length so
    that the padded copies stay small."""
    n = len(rows)
    lens = np.array([len(r) for r in rows], dtype=np.int64)
    mm, cm = np.zeros(n, np.uint32), np.zeros(n, np.uint32)
    klass = np.zeros(n, np.int64)
    for k in range(1, 16):
        klass[lens > (64 << (2 * (k - 1)))] = k
    for k in np.unique(klass):
        idx = np.nonzero(klass == k)[0]
        pad = np.zeros((idx.size, max(1, int(lens[idx].max()))), dtype=dtype)
        for j, i in enumerate(idx):
            pad[j, :lens[i]] = rows[i]
        L = lens[idx].astype(np.uint32)
        for i, o in enumerate(oracles):
            mm[idx] |= o.batch_matches(pad, L, threads=8).astype(np.uint32) << np.uint32(i)
            cm[idx] |= o.batch_contained_in(pad, L, threads=8).astype(np.uint32) << np.uint32(i)
    return mm, cm


def walk_tables(t, row, op):
    """One row through one group's product as PatternSet.tables() returns it: matches -- the mask of the state at the row's end;
    containedIn -- masks[start] OR masks[state] after every char."""
    cm, table, masks = t["class_map"], t["table"], t["masks"]
    st = t["start"]
    if op == "matches":
        for c in row:
            st = table[st, cm[c]]
            if st < 0:
                return 0
        return int(masks[st])
    m = int(masks[st])
    for c in row:
        st = table[st, cm[c]]
        m |= int(masks[st])
    return m


LENGTHS = [0, 1, 2, 3, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257]
LENGTHS_LONG = LENGTHS + [300, 523]  # (rows that hold a 261-char match with text around it)
LONG_ROWS = {70: 6000, 71: 9000}


def gpu_batch(name, seed=8, dtype=None, lengths=None, piece_every=7):
    """The batch recipe of the GPU tests, one for both char widths: 257 rows (a partial last group of 64), lengths cycling through
    LENGTHS, row 70 of 6000 and row 71 of 9000 chars (state and mask carried over 4 KiB and 8 KiB window edges), rows 128 .. 191 all
    empty (a group with no text), every other 7th row exactly one planted piece (a whole-row match; the pieces in turn, 27 such rows), a
    piece planted in half of the others (it fills a row of its own length: with ten pieces the default seed is one that gives every
    logs8 pattern its third whole-row match -- assert_batch_exercises_the_set checks what the batch holds).  The defaults are that
    recipe; dtype: rows of another char width (alphabet_and_pieces), lengths: "long" cycles through LENGTHS_LONG, piece_every: a
    whole-row piece every so many rows -- what GPU_RECIPE gives the sets that need it."""
    alphabet, pieces = alphabet_and_pieces(name, dtype)
    dtype = SETS[name][1] if dtype is None else dtype
    lengths = LENGTHS_LONG if lengths == "long" else LENGTHS if lengths is None else lengths
    rng = np.random.default_rng(seed)
    alpha = units(alphabet, dtype)
    rows = []
    planted = 0
    for r in range(257):
        n = LONG_ROWS.get(r, lengths[r % len(lengths)])
        if 128 <= r < 192:
            rows.append(np.zeros(0, dtype))
        elif r % piece_every == 0 and r not in LONG_ROWS:  # (row 70 is a long row, not a planted piece); the pieces in turn
            rows.append(units(pieces[planted % len(pieces)], dtype))
            planted += 1
        else:
            row = rng.choice(alpha, n).astype(dtype)
            if n and rng.random() < 0.5:
                w = units(pieces[int(rng.integers(len(pieces)))], dtype)
                if w.size <= n:
                    at = int(rng.integers(0, n - w.size + 1))
                    row[at:at + w.size] = w
            rows.append(row)
    assert len(rows) == 257 and all(rows[r].size == n for r, n in LONG_ROWS.items()) and not any(rows[r].size for r in range(128, 192))
    return rows


def assert_batch_exercises_the_set(name, want_m, want_c, k, nullable=()):
    """From the ORACLE's masks: every bit is set in >= 3 rows for both ops and clear in >= 1 row (a nullable pattern's containedIn bit is
    set in all)."""
    for i in range(k):
        cm, cc = int(((want_m >> np.uint32(i)) & 1).sum()), int(((want_c >> np.uint32(i)) & 1).sum())
        assert cm >= 3 and cc >= 3, (name, i, cm, cc)
        assert cm < want_m.size, (name, i)
        assert cc == want_c.size if i in nullable else cc < want_c.size, (name, i, cc)


# ---- random sets: the generator of the CPU fuzz (test_pattern_set.py) and of the GPU fuzz (test_gpu_fuzz.py)
FUZZ_SIZES = [1, 2, 3, 4, 6, 8, 12, 32]
FUZZ_FOLD_CHARS = [0xB5, 0x3BC, 0x212A, 0x130, ord("k"), ord("K"), 0x3B1]  # MICRO SIGN, mu, KELVIN SIGN, I with dot, k, K, alpha
OPS_WIDTHS = [(op, cw) for op in ("matches", "contained_in") for cw in (1, 2)]


def fuzz_alphabet(dtype):
    """The chars of the single-pattern GPU fuzz and the fold partners; 8-bit rows: those below 256."""
    from test_gpu_fuzz import ALPHABET
    return np.array([c for c in ALPHABET + FUZZ_FOLD_CHARS if np.dtype(dtype) == np.uint16 or c < 256], dtype=dtype)


def random_set(rng):
    """One random set: 1 .. 32 members random_regex(rng) x rng.choice(FLAG_SETS), a member that does not compile drawn again ->
    (members [(regex, flags)], PatternSet or None, per-member oracles, {(op, cw): info()}).  The set is None when PatternSet(...) or
    an info() refuses it (the callers count those)."""
    from needle_amd.pattern import DFACompiler, PatternException, PatternSet
    from oracle.walker import Dfa, OraclePattern
    from test_compile_vs_python_restatement import FLAG_SETS, random_regex
    k = rng.choice(FUZZ_SIZES)
    members, pats, oracles = [], [], []
    while len(members) < k:
        regex, flags = random_regex(rng), rng.choice(FLAG_SETS)
        try:
            p = DFACompiler.compile(regex, "m%d" % len(members), flags)
        except (PatternException, ValueError):
            continue
        t = p.tables()
        d = {key: Dfa(t["class_map"], t["stride"], v["table"], v["accepting"], v["max_char"]) for key, v in t["dfas"].items()}
        members.append((regex, flags))
        pats.append(p)
        oracles.append(OraclePattern(d["matches"], d["contained_in"], d["forwards"], d["backwards"], t["fixed_len"], -1))
    try:
        ps = PatternSet(pats)
        infos = {(op, cw): ps.info(op, cw) for op, cw in OPS_WIDTHS}
    except PatternException:
        return members, None, oracles, {}
    return members, ps, oracles, infos


def fuzz_counters(infos):
    """(TABLE16 plans, 1 if some plan has several groups) of one set's infos."""
    return (sum(g["kernel_mode"] == 2 for i in infos.values() for g in i["groups"]), int(any(i["n_groups"] > 1 for i in infos.values())))


# ---- what PatternSet.info() must report for the named sets: per set, in the order of OPS_WIDTHS (matches cw 1, matches cw 2,
# containedIn cw 1, containedIn cw 2), the product's n_states and kernel_mode (1: 8-bit table elements, 2: 16-bit), and the bounds
# (above, at most) of lds_bytes.  All of them are one group.
TABLE8, TABLE16 = 1, 2
SMALL, BIG = (0, 32768), (65536, 98304)  # 16 waves x 128-byte windows | 16 waves x 64-byte windows (ladder_shape)
PLANS = {
    "edge255": ([255] * 4, [TABLE8] * 4, [(0, 4096)] * 4),
    "edge256": ([256] * 4, [TABLE16] * 4, [(0, 6144)] * 4),
    "count260": ([271, 271, 268, 268], [TABLE16] * 4, [(0, 29696)] * 4),
    "count260ci": ([317, 318, 276, 278], [TABLE16] * 4, [(0, 29696)] * 4),
    "tail5": ([4098, 4098, 545, 545], [TABLE16] * 4, [BIG, BIG, SMALL, SMALL]),
    "mix16": ([162, 162, 642, 642], [TABLE8, TABLE8, TABLE16, TABLE16], [SMALL, SMALL, BIG, BIG]),
}
OLDER_GPU_SETS = ["nullable4", "logs8", "u16b", "kw32"]  # every plan of theirs: TABLE8 within SMALL


def ladder_shape(lds_bytes):
    """(waves, window bytes per row) of a plain table program of that size: the ladder of shape_for_program (needle_kernels.hip), the
    first rung whose windows fit the 160 KiB of LDS beside the program."""
    p = (lds_bytes + 15) & ~15
    for waves, chb in ((16, 128), (12, 128), (16, 64), (14, 64), (12, 64), (10, 64), (8, 64), (4, 64)):
        if p + waves * 64 * chb <= 160 * 1024:
            return waves, chb
    return None


def assert_plan(name, ps, op, cw):
    """info() of the plan about to run is the one PLANS lists: a lowering change cannot silently move a test to another kernel."""
    g = ps.info(op, cw)
    assert g["n_groups"] == 1, (name, op, cw, g)
    g = g["groups"][0]
    states, modes, bounds = (x[OPS_WIDTHS.index((op, cw))] for x in PLANS[name])
    assert (g["n_states"], g["kernel_mode"]) == (states, modes) and bounds[0] < g["lds_bytes"] <= bounds[1], (name, op, cw, g)
    return g
