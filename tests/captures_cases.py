"""What the capture tests share (test_captures_abi.py on the CPU, test_gpu_captures.py on the GPU): the reader of
tests/golden/captures.txt, the CPU walk of the tables that needle_pattern_captures_tables exports, the reference answers of `re`, the
must-work patterns with their texts, and the seeded pattern grammar of the fuzz."""
import os
import random
import re

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "captures.txt")

CASE_INSENSITIVE, LEFTMOST_LONGEST = 0x02, 0x800000
SRC_POS, SRC_NONE = -1, -2


def read_fixture(path=GOLDEN):
    """-> [(pattern, haystack, start, end, [group string or None, ...])]; '' and 'A' are quoted haystacks / strings, null is None."""
    unq = lambda s: s[1:-1] if len(s) >= 2 and s[0] == s[-1] == "'" else s
    rows = []
    with open(path, encoding="utf-8") as f:
        for line in f:
            line = line.strip()
            if not line or line.startswith("#"):
                continue
            pat, hay, start, end, caps = line.split()
            assert caps[0] == "[" and caps[-1] == "]"
            rows.append((pat, unq(hay), int(start), int(end), [None if c == "null" else unq(c) for c in caps[1:-1].split(",")]))
    return rows


def walk(t, text):
    """The walk of include/needle_hip.h on the tables `t` (Pattern.captures_tables) -> [(start, end)] for groups 0 .. G, or None where
    the pattern does not match `text` whole."""
    G2, slots = 2 * t["n_groups"], [-1] * max(t["n_slots"], 1)
    ops, op_off, cmap, nxt, opid = t["ops"], t["op_off"], t["class_map"], t["next"], t["op_id"]

    def run(k, pos):
        for i in range(op_off[k], op_off[k + 1]):
            dst, src = int(ops[i, 0]), int(ops[i, 1])
            slots[dst] = pos if src == SRC_POS else -1 if src == SRC_NONE else slots[src]
    run(t["init_op"], 0)
    st = t["start"]
    for i, ch in enumerate(text):
        c = cmap[ord(ch)]
        k, st = int(opid[st, c]), int(nxt[st, c])
        if st == 0:
            return None
        run(k, i + 1)
    f = int(t["fin"][st])
    if f < 0:
        return None
    return [(0, len(text))] + [(slots[f * G2 + 2 * g], slots[f * G2 + 2 * g + 1]) for g in range(t["n_groups"])]


def re_groups(cre, text):
    """re.fullmatch's spans for groups 0 .. G, or None."""
    m = cre.fullmatch(text)
    return None if m is None else [m.span(g) for g in range(cre.groups + 1)]


def to_re(pattern):
    """The regex for `re`: named groups are (?P<name> there."""
    return pattern.replace("(?<", "(?P<")


def clamp(s, e, n):
    s = min(max(s, 0), n)
    return s, min(max(e, s), n)


SENTINEL = -7


def reference_planes(groups_of, rows, span_off, start, end, n_groups):
    """What needle_captures_spans_packed_dev must write for a span list over `rows` (list of str): (gstart, gend) int32[G + 1, M] by
    groups_of(text) -- re_groups of a compiled `re`, or walk of the exported tables -- on the clamped spans; columns outside
    [span_off[0], span_off[-1]) hold SENTINEL."""
    m_all = len(start)
    gs, ge = np.full((n_groups + 1, m_all), SENTINEL, np.int32), np.full((n_groups + 1, m_all), SENTINEL, np.int32)
    for r, row in enumerate(rows):
        for m in range(int(span_off[r]), int(span_off[r + 1])):
            s, e = clamp(int(start[m]), int(end[m]), len(row))
            g = groups_of(row[s:e])
            for k in range(n_groups + 1):
                a, b = (-1, -1) if g is None or g[k][0] < 0 else (g[k][0] + s, g[k][1] + s)
                gs[k, m], ge[k, m] = a, b
    return gs, ge


SIXTEEN = "".join("(%s)" % c for c in "abcdefghijklmnop")
SEVENTEEN = SIXTEEN + "(q)"

# (regex, flags, char_width, texts): must be available; table walk == re.fullmatch on every text
MUST_WORK = [
    (r"([0-9]+)-([0-9]+)", 0, 1, ["1-2", "123-4567", "-", "12-", "-3", "1-2-3", "", "a-b", "00012-9"]),
    (r"(GET|POST|PUT) (/[^ ]*) HTTP/([0-9])\.([0-9])", 0, 1,
     ["GET / HTTP/1.1", "POST /a/b?c=d HTTP/2.0", "PUT /x HTTP/1.", "GET  HTTP/1.1", "HEAD / HTTP/1.1", "GET /a b HTTP/1.1", "PUT /é HTTP/0.9"]),
    (r"([0-9]{1,3})\.([0-9]{1,3})\.([0-9]{1,3})\.([0-9]{1,3})", 0, 1, ["1.2.3.4", "192.168.001.255", "1234.1.1.1", "1.2.3", "1..2.3", "10.0.0.1", "1.2.3.4567"]),
    (r"(?<year>[0-9]{4})-(?<mon>[0-9]{2})", 0, 1, ["2024-05", "2024-5", "02024-05", "abcd-ef", "1999-12"]),
    (r"(?:ab)+(c)", 0, 1, ["abc", "ababc", "c", "abab", "abcc", "aabc"]),
    (r"(.+)@(.+)", 0, 1, ["a@b", "a@b@c", "@", "a@", "@b", "user@example.com", "a@@b", "a\nb@c"]),
    (r"(a(b)?)+", 0, 1, ["aba", "a", "ab", "abab", "aab", "b", "", "abaa"]),
    (r"([^=&]+)=([^&]*)", 0, 1, ["k=v", "key=", "=v", "k=v=w", "a&b=c", "k=v&"]),
    (r"(\w+)@(\w+)\.com", 0, 1, ["joe@site.com", "joe@site.org", "j_1@S9.com", "@a.com", "a@.com", "a@b.comm"]),
    (SIXTEEN, 0, 1, ["abcdefghijklmnop", "abcdefghijklmno", "abcdefghijklmnopq", ""]),
    (r"[a-c]+x?", 0, 1, ["abcx", "x", "", "cab"]),  # G = 0
    ("([а-яё]+) ([一-龥]+)", 0, 2, ["привет 世界", "привет world", "ёж 龥", " 世界", "привет  世界", "abc 世界"]),
    (r"(get|post) (\S+)", CASE_INSENSITIVE, 1, ["GET /x", "get /x", "PoSt a b", "Post  ", "put /x", "gEt\t/x", "POST /a/b"]),
]

# (regex, reason)
MUST_REFUSE = [(SEVENTEEN, "TOO_MANY_GROUPS"), (r"(a*)+", "NULLABLE_LOOP"), (r"(a|b?)+", "NULLABLE_LOOP")]


def dictionary_regex(n=3000, seed=5):
    """n distinct keywords of 4 .. 9 lower-case letters in ONE group."""
    rng = random.Random(seed)
    words = set()
    while len(words) < n:
        words.add("".join(rng.choice("abcdefghijklmnopqrstuvwxyz") for _ in range(rng.randint(4, 9))))
    return "(" + "|".join(sorted(words)) + ")"


# ---- the fuzz grammar: patterns over `abc`, at most 8 leaves, 3 groups, depth 4, {m,n} with n <= 4; never a nullable loop body
class _Gen:
    def __init__(self, rng):
        self.rng, self.leaves, self.groups = rng, 0, 0

    def leaf(self):
        self.leaves += 1
        return self.rng.choice(["a", "b", "c", "[ab]", "[bc]", "[abc]", "."]), False

    def node(self, depth):
        """-> (regex of an atom-or-sequence, nullable)"""
        r = self.rng
        if depth >= 4 or self.leaves >= 8:
            return self.leaf()
        k = r.random()
        if k < 0.25:
            return self.leaf()
        if k < 0.45:  # concatenation
            parts = [self.node(depth + 1) for _ in range(r.randint(2, 3)) if self.leaves < 8] or [self.leaf()]
            return "".join(self.atom(p) if "|" in p else p for p, _ in parts), all(n for _, n in parts)
        if k < 0.62:  # alternation
            parts = [self.node(depth + 1) for _ in range(r.randint(2, 3)) if self.leaves < 8] or [self.leaf()]
            return "|".join(p for p, _ in parts), any(n for _, n in parts)
        if k < 0.80:  # group
            body, n = self.node(depth + 1)
            if self.groups < 3 and r.random() < 0.75:
                self.groups += 1
                return "(" + body + ")", n
            return "(?:" + body + ")", n
        body, n = self.node(depth + 1)
        body = self.atom(body)
        q = r.choice(["*", "+", "?", "{m,n}"])
        if q == "?":
            return body + "?", True
        if q == "{m,n}":
            hi = r.randint(1, 4)
            lo = r.randint(0, hi)
            if n and hi > 1:  # (a nullable body may repeat once at the most)
                return body + "?", True
            return body + "{%d,%d}" % (lo, hi), n or lo == 0
        if n:  # never a nullable loop body
            return body + "?", True
        return body + q, q == "*"

    @staticmethod
    def atom(p):
        """`p` as something a quantifier or a neighbour in a sequence binds to as a whole."""
        if len(p) == 1 or (p[0] == "[" and p.find("]") == len(p) - 1):
            return p
        if p[0] == "(" and _closes_at_end(p):
            return p
        return "(?:" + p + ")"


def _closes_at_end(p):
    depth = 0
    for i, ch in enumerate(p):
        depth += ch == "("
        depth -= ch == ")"
        if depth == 0:
            return i == len(p) - 1
    return False


def fuzz_patterns(count=2000, seed=20240607):
    rng = random.Random(seed)
    out = []
    while len(out) < count:
        g = _Gen(rng)
        p, _ = g.node(0)
        try:
            re.compile(p)
        except re.error:
            continue
        out.append(p)
    return out


def fuzz_texts(seed, count=100):
    """`count` texts over abc of length 0 .. 7 (all of the short ones first, then sampled)."""
    rng = random.Random(seed)
    texts = [""] + [c for c in "abc"] + [x + y for x in "abc" for y in "abc"]
    while len(texts) < count:
        texts.append("".join(rng.choice("abc") for _ in range(rng.randint(3, 7))))
    return texts[:count]
