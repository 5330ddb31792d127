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


def units(text, dtype):
    return np.array([ord(ch) for ch in text], dtype=dtype)


def compile_set(name):
    """(PatternSet, [per-pattern oracle], dtype) of a set above."""
    from needle_amd.pattern import DFACompiler, PatternSet
    from test_compile_matches_txt import oracle_for
    pats, dtype = SETS[name][0], SETS[name][1]
    return PatternSet([DFACompiler.compile(p, "p%d" % i, 0) for i, p in enumerate(pats)]), [oracle_for(p, 0)[0] for p in pats], dtype


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
LONG_ROWS = {70: 6000, 71: 9000}


def gpu_batch(name, seed=8):
    """The batch recipe of the GPU tests, one for both char widths: 257 rows (a partial last group of 64), lengths cycling through
    LENGTHS, row 70 of 6000 and row 71 of 9000 chars (state and mask carried over 4 KiB and 8 KiB window edges), rows 128 .. 191 all
    empty (a group with no text), every other 7th row exactly one planted piece (a whole-row match; the pieces in turn, 27 such rows), a
    piece planted in half of the others (it fills a row of its own length: with ten pieces the default seed is one that gives every
    logs8 pattern its third whole-row match -- assert_batch_exercises_the_set checks what the batch holds)."""
    _, dtype, alphabet, pieces = SETS[name]
    rng = np.random.default_rng(seed)
    alpha = units(alphabet, dtype)
    rows = []
    planted = 0
    for r in range(257):
        n = LONG_ROWS.get(r, LENGTHS[r % len(LENGTHS)])
        if 128 <= r < 192:
            rows.append(np.zeros(0, dtype))
        elif r % 7 == 0 and r not in LONG_ROWS:  # (row 70 is a long row, not a planted piece); the pieces in turn
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
