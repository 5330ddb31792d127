"""The UTF-8 rule of include/needle_hip.h in plain Python, and the batches the tests of the UTF-8 entries share (test_utf8_abi.py on the
CPU, test_gpu_utf8.py on the GPU).  utf8_units is the reference every GPU comparison is bit-exact against; test_utf8_abi.py pins it to
CPython's bytes.decode("utf-8", "replace")."""
import itertools
import random

import numpy as np

ALPHABET = bytes.fromhex("00 41 7F 80 8F 90 9F A0 BF C0 C1 C2 DF E0 E1 EC ED EE EF F0 F1 F3 F4 F5 FF")

NEED = [2 if 0xC2 <= b <= 0xDF else 3 if 0xE0 <= b <= 0xEF else 4 if 0xF0 <= b <= 0xF4 else 0 for b in range(256)]
CONT = [0x80 <= b <= 0xBF for b in range(256)]
_SECOND = {0xE0: (0xA0, 0xBF), 0xED: (0x80, 0x9F), 0xF0: (0x90, 0xBF), 0xF4: (0x80, 0x8F)}


def second_ok(lead, b):
    lo, hi = _SECOND.get(lead, (0x80, 0xBF))
    return lo <= b <= hi


def utf8_units(row):
    """(units, starts): the UTF-16 code units the row files and the byte offsets of the bytes that start something -- one entry of
    `starts` per start, so a complete 4-byte sequence has ONE start and TWO units."""
    row = bytes(row)
    n, units, starts = len(row), [], []
    for i, b in enumerate(row):
        if CONT[b] and ((i >= 1 and NEED[row[i - 1]] >= 2 and second_ok(row[i - 1], b))
                        or (i >= 2 and NEED[row[i - 2]] >= 3 and second_ok(row[i - 2], row[i - 1]))
                        or (i >= 3 and NEED[row[i - 3]] == 4 and second_ok(row[i - 3], row[i - 2]) and CONT[row[i - 1]])):
            continue  # consumed
        starts.append(i)
        if b < 0x80:
            units.append(b)
            continue
        k = NEED[b]
        if k and i + k <= n and second_ok(b, row[i + 1]) and all(CONT[row[j]] for j in range(i + 2, i + k)):
            cp = b & (0x1F if k == 2 else 0x0F if k == 3 else 0x07)
            for j in range(i + 1, i + k):
                cp = (cp << 6) | (row[j] & 0x3F)
            if k == 4:
                cp -= 0x10000
                units.extend((0xD800 | (cp >> 10), 0xDC00 | (cp & 0x3FF)))
            else:
                units.append(cp)
        else:
            units.append(0xFFFD)
    return units, starts


def _unit_bytes(row, units, starts):
    out, u = [], 0
    for s in starts:
        two = 0xD800 <= units[u] < 0xDC00 and NEED[row[s]] == 4  # (U+FFFD and 3-byte code points are never in the surrogate range)
        out.extend((s, s) if two else (s,))
        u += 2 if two else 1
    assert u == len(units)
    return out + [len(row)]


def unit_bytes(row):
    """B(0 .. U) of the row: the byte offset of the start that files each unit (both units of a pair: the sequence's start), then len."""
    return _unit_bytes(row, *utf8_units(row))


def byte_of_unit(row, p):
    """B(p): -1 for a negative p, len for p >= U."""
    if p < 0:
        return -1
    b = unit_bytes(row)
    return b[min(p, len(b) - 1)]


# ---- batches
def alphabet_rows():
    """Every row of 1 to 4 alphabet bytes: 406 900 rows, 1.6 MB."""
    return [bytes(t) for k in (1, 2, 3, 4) for t in itertools.product(ALPHABET, repeat=k)]


def random_rows(n, seed, max_len=11):
    rng = random.Random(seed)
    pool = ALPHABET + bytes(range(256))
    return [bytes(rng.choice(pool) for _ in range(rng.randrange(0, max_len + 1))) for _ in range(n)]


_CHARS = {"ascii": lambda r: chr(r.randrange(0x20, 0x7F)), "cyrillic": lambda r: chr(r.randrange(0x430, 0x450)),
          "cjk": lambda r: chr(r.randrange(0x4E00, 0x4F00)), "astral": lambda r: chr(r.randrange(0x1F600, 0x1F650))}
_ILL = [b"\x80", b"\xC0\xAF", b"\xE2\x82", b"\xED\xA0\x80", b"\xF0\x9F\x98", b"\xF5", b"\xFF", b"\xF4\x90\x80\x80", b"\xE0\x80\x80"]


def mixed_bytes(n_chars, rng, weights=(70, 15, 10, 4, 1), words=()):
    """Seeded text: per character ASCII / Cyrillic / CJK / astral / an ill-formed piece by `weights`, with `words` planted here and there."""
    out = []
    kinds = ("ascii", "cyrillic", "cjk", "astral", "ill")
    for k in rng.choices(kinds, weights=weights, k=n_chars):
        if words and rng.random() < 0.08:
            out.append(rng.choice(words).encode("utf-8"))
        out.append(rng.choice(_ILL) if k == "ill" else _CHARS[k](rng).encode("utf-8"))
    return b"".join(out)


def long_row(n_bytes, seed):
    """Mixed 1- / 2- / 3- / 4-byte text of exactly n_bytes with an ill-formed byte at every 997th position."""
    rng = random.Random(seed)
    out = bytearray()
    while len(out) < n_bytes:
        out += _CHARS[rng.choice(("ascii", "ascii", "cyrillic", "cjk", "astral"))](rng).encode("utf-8")
    out = out[:n_bytes]
    for i in range(996, n_bytes, 997):
        out[i] = (0x80, 0xFF, 0xC0, 0xE2, 0xF0)[(i // 997) % 5]
    return bytes(out)


def bitmap(flags):
    """bool[n] -> the library's bitmap words (bit r of word r / 64; the bits at or above n are 0)."""
    flags = np.asarray(flags, bool)
    padded = np.zeros((flags.size + 63) // 64 * 64, np.uint8)
    padded[:flags.size] = flags
    return np.packbits(padded, bitorder="little").view(np.uint64)


class Expected:
    """What the entries must give for `rows`: lengths, the units back to back, the per-row flags of both bitmaps, and B(0 .. U) of
    every row (`byte_maps`)."""

    def __init__(self, rows):
        self.rows = list(rows)
        self.lengths, self.non_ascii, self.malformed, self.byte_maps, units_all, seen = [], [], [], [], [], {}
        for row in self.rows:
            got = seen.get(row)
            if got is None:
                units, starts = utf8_units(row)
                # (EF BF BD always decodes to a genuine U+FFFD: EF is never a continuation byte.  Any U+FFFD beyond those was substituted.)
                got = seen[row] = (units, _unit_bytes(row, units, starts), any(b >= 0x80 for b in row), units.count(0xFFFD) > row.count(b"\xEF\xBF\xBD"))
            self.lengths.append(len(got[0]))
            units_all.extend(got[0])
            self.byte_maps.append(got[1])
            self.non_ascii.append(got[2])
            self.malformed.append(got[3])
        self.lengths = np.array(self.lengths, np.int64)
        self.units = np.array(units_all, np.uint16)

    @staticmethod
    def join(a, b):
        """The batch of a's rows followed by b's."""
        e = Expected([])
        e.rows = a.rows + b.rows
        e.lengths = np.concatenate([a.lengths, b.lengths])
        e.units = np.concatenate([a.units, b.units])
        e.non_ascii, e.malformed, e.byte_maps = a.non_ascii + b.non_ascii, a.malformed + b.malformed, a.byte_maps + b.byte_maps
        return e

    def unit_offsets(self, first=0):
        off = np.full(len(self.rows) + 1, first, np.int64)
        off[1:] += np.cumsum(self.lengths)
        return off

    def position_list(self, rows=None, extra=(), order=None, first=0, cap=None):
        """A CSR list over the rows and its answers: for every row of `rows` (default: all) the positions 0 .. U (cap: at most that
        many of them, a seeded sample) and `extra(U)`; order: None | "reversed" | a random.Random to shuffle each row's entries with.
        -> (list_offsets, unit_pos, byte_pos); the first `first` entries belong to no row."""
        pick = set(range(len(self.rows))) if rows is None else set(rows)
        off, pos, ans = [first], [0] * first, [0] * first
        for r, bm in enumerate(self.byte_maps):
            if r in pick:
                u = len(bm) - 1
                ps = list(range(u + 1)) if cap is None or u < cap else sorted(random.Random(u).sample(range(u + 1), cap))
                ps += list(extra(u) if callable(extra) else extra)
                if order == "reversed":
                    ps.reverse()
                elif order is not None:
                    order.shuffle(ps)
                pos.extend(ps)
                ans.extend(-1 if p < 0 else bm[min(p, u)] for p in ps)
            off.append(len(pos))
        return np.array(off, np.int64), np.array(pos, np.int32), np.array(ans, np.int32)


def device_utf8(rows, lead=b"", shift=0):
    """The rows on the device between sentinels: a leading sentinel that ENDS in E2 82 (`shift` more sentinel bytes move the text's
    alignment), `lead` rows' worth of pad bytes are the caller's business; a trailing sentinel that STARTS with AC.  -> (data uint8 tensor
    padded to whole 4 bytes, offsets int64 tensor with offsets[0] > 0, host copy of data)."""
    import torch
    front = b"\x5A" * (14 + shift) + b"\xE2\x82"
    body = b"".join(rows)
    back = b"\xAC" + b"\x5A" * 19
    host = np.frombuffer(front + body + back, np.uint8)
    host = np.concatenate([host, np.full((-host.size) % 4, 0x5A, np.uint8)])
    offsets = np.zeros(len(rows) + 1, np.int64)
    offsets[1:] = np.cumsum([len(r) for r in rows])
    offsets += len(front)
    return torch.from_numpy(host.copy()).to("cuda"), torch.from_numpy(offsets).to("cuda"), host
