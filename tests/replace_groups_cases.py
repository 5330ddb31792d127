"""What the template-replacement tests share (test_replace_groups_abi.py on the CPU, test_gpu_replace_groups.py on the GPU): the template
parser restated from the rules of include/needle_hip.h (not from the C code), the expansion of a parsed template on one match, the
definition of the splice with its clamps, and seeded templates."""
import random
import re

import numpy as np

from captures_cases import clamp, fuzz_patterns

MAX_REFS, MAX_UNITS = 16, 4096
# Of fuzz_chosen()'s 200 patterns, those whose captures are refused (captures_info, no device): test_replace_groups_abi.py counts them on
# the CPU, test_gpu_replace_groups.py leaves exactly those out.  The cap is 1 % of the patterns.
FUZZ_REFUSED, FUZZ_REFUSED_CAP = 0, 2


def fuzz_chosen(count=200):
    """(index, regex) of the first `count` patterns of the capture fuzz that have at least one group."""
    return [(i, rx) for i, rx in enumerate(fuzz_patterns()) if re.compile(rx).groups > 0][:count]


def parse(t, G):
    """A template (str, or list of UTF-16 code units) for a pattern with G groups -> (groups, literals as lists of code units), or the
    str "error"."""
    t = [ord(c) for c in t] if isinstance(t, str) else list(t)
    groups, lits, i = [], [[]], 0
    while i < len(t):
        if t[i] == ord("\\"):
            if i + 1 == len(t):
                return "error"
            lits[-1].append(t[i + 1])
            i += 2
        elif t[i] == ord("$"):
            if i + 1 == len(t) or not 48 <= t[i + 1] <= 57 or t[i + 1] - 48 > G:
                return "error"
            g, i = t[i + 1] - 48, i + 2
            while i < len(t) and 48 <= t[i] <= 57 and g * 10 + t[i] - 48 <= G:
                g, i = g * 10 + t[i] - 48, i + 1
            groups.append(g)
            lits.append([])
        else:
            lits[-1].append(t[i])
            i += 1
    return "error" if len(groups) > MAX_REFS or sum(len(x) for x in lits) > MAX_UNITS else (groups, lits)


def units_str(u):
    return np.asarray(u, np.uint16).tobytes().decode("utf-16-le", "surrogatepass")


def expand(groups, literals, row, spans):
    """literals[0] + row[span of groups[0]] + literals[1] + ...: `spans` holds (start, end) per group, relative to `row`; a group with
    start < 0 (or None) contributes nothing.  str rows with str literals, numpy rows with array literals."""
    parts = [literals[0]]
    for g, lit in zip(groups, literals[1:]):
        sp = spans[g]
        if sp is not None and sp[0] >= 0:
            x, y = clamp(sp[0], sp[1], len(row))
            parts.append(row[x:y])
        parts.append(lit)
    if isinstance(row, np.ndarray):
        return np.concatenate([np.asarray(p, dtype=row.dtype) for p in parts])
    return "".join(parts)


def splice_groups(row, planes_of_row, groups, literals):
    """The definition (include/needle_hip.h): planes_of_row = one list of (start, end) for planes 0 .. n_planes - 1 per match of the row.
    A match whose plane 0 starts below 0 is KEPT and is no piece at all; every other is clamped into the row and replaced by its
    expansion; the text between the replaced matches stays."""
    n, parts, pos = len(row), [], 0
    for spans in planes_of_row:
        if spans[0][0] < 0:
            continue
        s, e = clamp(spans[0][0], spans[0][1], n)
        parts += [row[pos:s], expand(groups, literals, row, spans)]
        pos = e
    parts.append(row[pos:])
    if isinstance(row, np.ndarray):
        return np.concatenate([np.asarray(p, dtype=row.dtype) for p in parts])
    return "".join(parts)


def random_template(rng, alphabet="$\\{}019ab", max_len=8):
    return "".join(rng.choice(alphabet) for _ in range(rng.randint(0, max_len)))


def seeded_templates(seed, G, count):
    """`count` templates that parse for G groups, with literals of `<>-x` and up to five references."""
    rng, out = random.Random(seed), []
    while len(out) < count:
        t = ""
        for _ in range(rng.randint(0, 5)):
            t += "".join(rng.choice("<>-x") for _ in range(rng.randint(0, 3))) + "$%d" % rng.randint(0, G)
        t += "".join(rng.choice("<>-x") for _ in range(rng.randint(0, 3)))
        if parse(t, G) != "error":
            out.append(t)
    return out
