"""The chunk arithmetic of the host-buffer entries (needle_amd/csrc/needle_host_plan.h) on the CPU: tests/c/host_plan_check.cpp, a
stand-alone program built with -fsanitize=address,undefined, against the rules restated here, and the properties the entries rely on."""
import os
import random
import subprocess

import pytest

from conftest import ROOT


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("host_plan") / "host_plan_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "c", "host_plan_check.cpp"), "-o", exe])

    def run(cases):
        text = "".join(" ".join(str(x) for x in c) + "\n" for c in cases)
        r = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr[-4000:]
        lines = r.stdout.split("\n")[:-1]
        assert len(lines) == len(cases)
        return [[int(x) for x in ln.split()] for ln in lines]
    return run


def pairs(flat):
    return list(zip(flat[0::2], flat[1::2]))


# ---- the rules, restated
def up16(x):
    return (x + 15) & ~15


def padded_stride(row_stride, cw):
    return max(16, up16(row_stride * cw))


def fixed_rows(stride, per_row, budget):
    return max(64, (budget // (stride + per_row)) & ~63)


def packed_chunks(off, cw, per_row, align, budget):
    n, chunks, r0 = len(off) - 1, [], 0
    while r0 < n:
        r1 = min(r0 + align, n)
        while r1 < n:
            nxt = min(r1 + align, n)
            if (off[nxt] - off[r0]) * cw + (nxt - r0) * per_row > budget:
                break
            r1 = nxt
        chunks.append((r0, r1))
        r0 = r1
    return chunks


def csr_ranges(off, r0, r1, max_m):
    ranges, a = [], r0
    while a < r1:
        b = a + 1
        while b < r1 and off[b + 1] - off[a] <= max_m:
            b += 1
        ranges.append((a, b))
        a = b
    return ranges


def random_offsets(rng, n, first=None):
    off = [rng.randrange(1, 1000) if first is None else first]
    for _ in range(n):
        off.append(off[-1] + (50000 if rng.random() < 0.002 else rng.randrange(0, 301)))
    return off


def check_partition(chunks, n):
    assert [a for a, _ in chunks] == ([0] + [b for _, b in chunks[:-1]] if n else []) and all(a < b for a, b in chunks)
    assert (chunks[-1][1] if chunks else 0) == n


def check_packed(chunks, off, cw, per_row, align, budget):
    n = len(off) - 1
    check_partition(chunks, n)
    for a, b in chunks:
        assert b - a >= min(align, n - a)  # at least `align` rows, or the rest
        if align == 64:
            assert a % 64 == 0
        if (off[b] - off[a]) * cw + (b - a) * per_row > budget:
            assert b - a == min(align, n - a)  # above the budget: of minimum size


def test_strides_and_fixed_chunks(plan):
    rng = random.Random(1)
    s_cases = [(s, cw) for cw in (1, 2) for s in list(range(0, 40)) + [rng.randrange(0, 70000) for _ in range(100)]]
    for (s, cw), (got,) in zip(s_cases, plan([("stride", s, cw) for s, cw in s_cases])):
        assert got == padded_stride(s, cw) and got % 16 == 0 and got >= 16 and got >= s * cw
    f_cases = [(padded_stride(rng.randrange(0, 2000), rng.choice((1, 2))), rng.choice((0, 16, 8 + 8 * rng.randrange(0, 9))),
                rng.choice((0, 1, 4096, 20000, 1 << 20, 2 << 30, rng.randrange(0, 1 << 34)))) for _ in range(200)]
    for (s, pr, b), (got,) in zip(f_cases, plan([("fixed", s, pr, b) for s, pr, b in f_cases])):
        assert got == fixed_rows(s, pr, b) and got % 64 == 0 and got >= 64
        assert got == 64 or got * (s + pr) <= b
    # the chunk sizes the GPU tests' comments state (NEEDLE_HOST_CHUNK_BYTES = 1 MiB)
    assert plan([("fixed", 256, 0, 1 << 20), ("fixed", 128, 0, 1 << 20)]) == [[4096], [8192]]


def test_packed_chunks(plan):
    rng = random.Random(2)
    cases = []
    for i in range(200):
        n = (0, 1, 63, 64, 65)[i % 5] if i < 10 else rng.randrange(0, 5001)
        align, per_row = rng.choice(((64, 8 + 4), (64, 8 + 2), (1, 12), (64, padded_stride(300, 1) + 20)))
        cases.append((rng.choice((1, 2)), per_row, align, rng.choice((0, 4096, 20000, 100000, 1 << 20, 2 << 30)), random_offsets(rng, n)))
    for n in (0, 1, 63, 64, 65, 200):
        for align in (1, 64):
            cases.append((1, 12, align, 20000, [7] * (n + 1)))                     # all rows empty
            cases.append((2, 12, align, 0, random_offsets(rng, n)))                # budget 0: terminates, chunks of `align` rows
            cases.append((1, 12, align, 1000, random_offsets(rng, n // 2) + [10 ** 6 + 10 ** 5 * k for k in range(n - n // 2)]))  # rows larger than the budget
    got = plan([("packed", cw, pr, al, b, len(off) - 1, *off) for cw, pr, al, b, off in cases])
    for (cw, pr, al, b, off), flat in zip(cases, got):
        chunks = pairs(flat)
        assert chunks == packed_chunks(off, cw, pr, al, b)
        check_packed(chunks, off, cw, pr, al, b)
        if b == 0:
            n = len(off) - 1
            assert all(c1 - c0 == min(al, n - c0) for c0, c1 in chunks)
        if b == 2 << 30:
            assert len(chunks) <= 1  # a batch within the budget: exactly one chunk


def test_csr_ranges(plan):
    rng = random.Random(3)
    cases = []
    for i in range(200):
        n = (0, 1, 63, 64, 65)[i % 5] if i < 10 else rng.randrange(0, 5001)
        off = random_offsets(rng, n, first=rng.choice((0, 0, 12345)))
        r0 = rng.randrange(0, n + 1)
        cases.append((r0, rng.randrange(r0, n + 1), rng.choice((1, 100, 1024, 50000, 1 << 26)), off))
    cases.append((0, 3, 10, [0, 4, 40, 44]))    # a row with more matches than max_m: a range of its own
    cases.append((0, 5, 1, [0, 0, 0, 0, 0, 0]))  # no matches at all
    got = plan([("csr", r0, r1, mm, len(off) - 1, *off) for r0, r1, mm, off in cases])
    for (r0, r1, mm, off), flat in zip(cases, got):
        ranges = pairs(flat)
        assert ranges == csr_ranges(off, r0, r1, mm)
        assert [a for a, _ in ranges] == ([r0] + [b for _, b in ranges[:-1]] if r1 > r0 else []) and (ranges[-1][1] if ranges else r0) == r1
        for a, b in ranges:
            assert b > a and (off[b] - off[a] <= mm or b == a + 1)
    assert pairs(got[-2]) == [(0, 1), (1, 2), (2, 3)]


def test_length_classes_and_slab(plan):
    rng = random.Random(4)
    lens = list(range(0, 70)) + [64 << (2 * k) for k in range(12)] + [(64 << (2 * k)) + 1 for k in range(12)] + [rng.randrange(0, 1 << 33) for _ in range(100)]
    for b, (k,) in zip(lens, plan([("class", b) for b in lens])):
        assert b <= 64 << (2 * k) and (k == 0 or b > 64 << (2 * (k - 1)))
    slabs = [[rng.choice((0, 1, 4, 15, 16, 17, rng.randrange(0, 100000))) for _ in range(rng.randrange(0, 9))] for _ in range(200)]
    for sizes, flat in zip(slabs, plan([("slab", len(s), *s) for s in slabs])):
        offs, total, end = flat[:-1], flat[-1], 0
        for o, b in zip(offs, sizes):
            assert o % 16 == 0 and o == up16(end)  # no overlap, no more than the alignment between two sections
            end = o + b
        assert total == end
