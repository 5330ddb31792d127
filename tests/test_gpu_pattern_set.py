"""Pattern sets on the GPU (needle_set_*_packed_dev / _host, the kernel of needle_packed_set.h): both ops against the oracle per pattern on
every row of one small batch recipe (pattern_set_cases.gpu_batch) for 8-bit and UTF-16 rows -- sets with 8- and with 16-bit table
elements, on both sides of the boundary between them, with programs small enough for 128-byte windows and too big for them, and with
other workgroup shapes forced --, several groups with the table budget lowered, the host entries in several chunks, and 10^5 rows of a
32-keyword set against the 32 single-pattern scans."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT
from pattern_set_cases import (GPU_RECIPE, KW32, PLANS, SETS, assert_batch_exercises_the_set, assert_plan, compile_set, gpu_batch, oracle_masks,
                               split_case, units)

pytestmark = pytest.mark.gpu

JUNK = {"nullable4": "abc123x", "logs8": "42 ERROR a-c Holmes ", "u16b": "αβγεab一二", "edge255": "a", "edge256": "a", "count260": "efgx42 ab bcdy",
        "count260ci": "EFGX42 aB BcDy KELVIN", "tail5": "a12345", "mix16": "42 ERROR a-c Holmes 0x1f [42]"}
NEW_CASES = [s + w for s in ("edge255", "edge256", "count260", "count260ci", "tail5", "mix16") for w in ("@8", "@16")]


@pytest.fixture(scope="module", autouse=True)
def built():
    from needle_amd import build
    build.build()
    from oracle import walker
    walker.build()


_cache = {}


def case(case):
    """(set, per-pattern oracles, dtype, rows, oracle matches masks, oracle containedIn masks) of "name" or "name@8" / "name@16"
    (pattern_set_cases.split_case) -- computed once."""
    if case not in _cache:
        name, dtype = split_case(case)
        ps, oracles, dtype = compile_set(name, dtype)
        rows = gpu_batch(name, dtype=dtype, **GPU_RECIPE.get(name, {}))
        _cache[case] = (ps, oracles, dtype, rows) + oracle_masks(oracles, rows, dtype)
    return _cache[case]


def device_masks(ps, data, offsets, n, garbage=False):
    import torch
    out_m = out_c = None
    if garbage:  # group 0 must STORE the masks, not OR into what the caller left there
        out_m = torch.full((n,), -1, dtype=torch.int32, device="cuda")
        out_c = torch.full((n,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    m = ps.matches_packed(data, offsets, out=out_m)
    c = ps.contained_in_packed(data, offsets, out=out_c)
    torch.cuda.synchronize()
    assert m.is_cuda and m.dtype == torch.int32 and m.numel() == n
    return m.cpu().numpy().view(np.uint32), c.cpu().numpy().view(np.uint32)


def check_masks(name, got_m, got_c, want_m, want_c, rows, k, what=""):
    for op, got, want in (("matches", got_m, want_m), ("containedIn", got_c, want_c)):
        bad = np.nonzero(got != want)[0]
        assert bad.size == 0, (name, what, op, bad[:10], [len(rows[i]) for i in bad[:10]], got[bad[:5]], want[bad[:5]])
        assert not (got >> np.uint32(k)).any(), (name, what, op, "bits at or above n_patterns")


def assert_edge_rows(name, rows):
    """edge255 / edge256: runs of 0, 1 and 253 .. 257 `a`s as whole rows, and 254 `a`s with a `b` behind and in front."""
    texts = {"".join(chr(c) for c in r.tolist()) for r in rows if r.size <= 258}
    for want in ["a" * n for n in (0, 1, 253, 254, 255, 256, 257)] + ["a" * 254 + "b", "b" + "a" * 254]:
        assert want in texts, (name, len(want), want[:1], want[-1:])


@pytest.mark.parametrize("name", ["nullable4", "logs8", "u16b"] + NEW_CASES)
def test_set_masks_equal_the_oracle_per_pattern(name):
    """(The cases of NEW_CASES: both ops x both char widths with 16-bit table elements -- all but edge255 and mix16's matches --, with
    64-byte windows -- tail5's matches and mix16's containedIn programs are above 64 KB: windows of 4 KiB a wave, which the 6000- and
    9000-char rows cross at other places --, and the last 8-bit / first 16-bit program, edge255 / edge256.)"""
    from test_gpu_packed_dev import device_packed
    ps, oracles, dtype, rows, want_m, want_c = case(name)
    name = split_case(name)[0]
    k = len(oracles)
    assert_batch_exercises_the_set(name, want_m, want_c, k, nullable=(0,) if name == "nullable4" else ())
    if name in PLANS:  # the plans about to run are the ones this case is here for
        for op in ("matches", "contained_in"):
            assert_plan(name, ps, op, np.dtype(dtype).itemsize)
    if name.startswith("edge"):
        assert_edge_rows(name, rows)
    # offsets[0] > 0, data only 4-byte aligned, the last row ends at the tensor's end
    data, offsets = device_packed(rows, dtype, lead=5, trail=0)
    assert int(offsets[0]) > 0 and int(offsets[-1]) == data.numel()
    got_m, got_c = device_masks(ps, data, offsets, len(rows))
    check_masks(name, got_m, got_c, want_m, want_c, rows, k, "zeros around")
    # text that matches the patterns before offsets[0] and after offsets[n]: an over-read changes answers
    data, offsets = device_packed(rows, dtype, lead=5, trail=7, junk=units(JUNK[name], dtype))
    got_m, got_c = device_masks(ps, data, offsets, len(rows), garbage=True)
    check_masks(name, got_m, got_c, want_m, want_c, rows, k, "junk around")


def run_child(code, env):
    out = subprocess.run([sys.executable, "-c", "import sys; sys.path.insert(0, %r); sys.path.insert(0, %r)\n" % (ROOT, os.path.join(ROOT, "tests")) + code],
                         env=dict(os.environ, **env), capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "CHILD OK" in out.stdout, (out.stdout[-2000:], out.stderr[-3000:])


SHAPE_CHILD = ("import numpy as np\n"
               "from oracle import walker; walker.build()\n"
               "from test_gpu_packed_dev import device_packed\n"
               "from test_gpu_pattern_set import JUNK, case, check_masks, device_masks\n"
               "from pattern_set_cases import split_case, units\n"
               "for c in ('logs8', 'logs8@16', 'count260', 'count260@16'):\n"
               "    ps, oracles, dtype, rows, want_m, want_c = case(c)\n"
               "    for op in ('matches', 'contained_in'):\n"
               "        mode = ps.info(op, np.dtype(dtype).itemsize)['groups'][0]['kernel_mode']\n"
               "        assert mode == (1 if c.startswith('logs8') else 2), (c, op, mode)\n"
               "    data, offsets = device_packed(rows, dtype, lead=5, trail=7, junk=units(JUNK[split_case(c)[0]], dtype))\n"
               "    got_m, got_c = device_masks(ps, data, offsets, len(rows), garbage=True)\n"
               "    check_masks(c, got_m, got_c, want_m, want_c, rows, len(oracles), 'forced shape')\n"
               "print('CHILD OK')\n")


@pytest.mark.parametrize("shape", ["16x64", "4x64", "12x128"])
def test_forced_workgroup_shapes(shape):
    """logs8 (8-bit table elements) and count260 (16-bit) on 8-bit and UTF-16 rows, both ops, with NEEDLE_SHAPE = <waves>x<window bytes
    per row> in a child process (the switch is read once per process): 64-byte windows under small programs, workgroups of 4 and of 12
    waves.  Nothing reports the shape that ran: the test knows only that the switch was set to a shape shape_for_program accepts for
    programs of this size (waves x 64 x window bytes beside them within 160 KiB)."""
    out = subprocess.run([sys.executable, "-c", "import sys; sys.path.insert(0, %r); sys.path.insert(0, %r)\n" % (ROOT, os.path.join(ROOT, "tests")) + SHAPE_CHILD],
                         env=dict(os.environ, NEEDLE_SHAPE=shape), capture_output=True, text=True, timeout=180)
    assert out.returncode == 0 and "CHILD OK" in out.stdout, (shape, out.stdout[-2000:], out.stderr[-3000:])


def test_several_groups_store_then_or():
    """The logs8 batch with the table budget lowered so that the set is cut into groups: the same masks, into a tensor pre-filled with
    garbage (group 0 stores, later groups read-modify-write)."""
    run_child("import numpy as np\n"
              "from oracle import walker; walker.build()\n"
              "from pattern_set_cases import compile_set, gpu_batch, oracle_masks\n"
              "from test_gpu_packed_dev import device_packed\n"
              "from test_gpu_pattern_set import device_masks, check_masks\n"
              "ps, oracles, dtype = compile_set('logs8')\n"
              "for op in ('matches', 'contained_in'):\n"
              "    assert ps.info(op, 1)['n_groups'] >= 2, ps.info(op, 1)\n"
              "rows = gpu_batch('logs8')\n"
              "want_m, want_c = oracle_masks(oracles, rows, dtype)\n"
              "data, offsets = device_packed(rows, dtype, lead=5, trail=0)\n"
              "got_m, got_c = device_masks(ps, data, offsets, len(rows), garbage=True)\n"
              "check_masks('logs8', got_m, got_c, want_m, want_c, rows, 8, 'groups')\n"
              "print('CHILD OK')\n", {"NEEDLE_MAX_PROG_LDS": "4096"})


def test_host_entries_and_strings_in_several_chunks():
    """needle_set_*_packed_host and *_strings on 300 strings with NEEDLE_HOST_CHUNK_BYTES small enough for several chunks (UTF-16 rows
    through pack_strings; 8-bit rows with offsets[0] > 0)."""
    run_child("import numpy as np\n"
              "from oracle import walker; walker.build()\n"
              "from pattern_set_cases import SETS, compile_set, gpu_batch, oracle_masks, units\n"
              "for name in ('u16b', 'logs8'):\n"
              "    ps, oracles, dtype = compile_set(name)\n"
              "    rows = [r for r in gpu_batch(name) if r.size < 300] + gpu_batch(name, seed=9)[:60]\n"
              "    rows = rows[:300]\n"
              "    assert len(rows) == 300 and sum(r.size for r in rows) * 2 > 3 * 4096\n"
              "    strings = [''.join(chr(int(c)) for c in r) for r in rows]\n"
              "    want_m, want_c = oracle_masks(oracles, [units(s, np.uint16) for s in strings], np.uint16)\n"
              "    assert (ps.matches_strings(strings) == want_m).all() and (ps.contained_in_strings(strings) == want_c).all(), name\n"
              "    if dtype == np.uint8:\n"
              "        lead = np.frombuffer(b'42 ERROR', dtype=np.uint8)\n"
              "        data = np.concatenate([lead] + rows)\n"
              "        offsets = np.cumsum([lead.size] + [r.size for r in rows]).astype(np.uint64)\n"
              "        assert (ps.matches_packed(data, offsets) == want_m).all() and (ps.contained_in_packed(data, offsets) == want_c).all()\n"
              "print('CHILD OK')\n", {"NEEDLE_HOST_CHUNK_BYTES": "4096"})


def test_kw32_against_the_single_pattern_scans():
    """10^5 rows: the set's containedIn() masks against the 32 single-pattern needle_contained_in_packed_dev bitmaps, and both ops against
    the oracle on a 2000-row sample."""
    import torch
    from needle_amd.pattern import DFACompiler, unpack_bitmap
    from test_gpu_packed_dev import device_packed
    ps, oracles, dtype = compile_set("kw32")
    rng = np.random.default_rng(11)
    n = 100000
    alpha = units(SETS["kw32"][2], dtype)
    lens = rng.integers(0, 97, n)
    rows = []
    for i in range(n):
        row = rng.choice(alpha, int(lens[i])).astype(dtype)
        for _ in range(int(rng.integers(0, 3))):
            w = units(KW32[int(rng.integers(32))], dtype)
            if w.size <= row.size:
                at = int(rng.integers(0, row.size - w.size + 1))
                row[at:at + w.size] = w
        rows.append(row)
    data, offsets = device_packed(rows, dtype, lead=5, trail=0)
    got_m, got_c = device_masks(ps, data, offsets, n)
    want = np.zeros(n, np.uint32)
    for i, w in enumerate(KW32):
        bm = DFACompiler.compile(w, "w%d" % i).contained_in_packed(data, offsets)
        torch.cuda.synchronize()
        want |= unpack_bitmap(bm, n).astype(np.uint32) << np.uint32(i)
    assert all(int(((want >> np.uint32(i)) & 1).sum()) >= 3 for i in range(32))
    bad = np.nonzero(got_c != want)[0]
    assert bad.size == 0, (bad[:10], got_c[bad[:5]], want[bad[:5]])
    sample = rng.choice(n, 2000, replace=False)
    sm, sc = oracle_masks(oracles, [rows[i] for i in sample], dtype)
    assert (got_m[sample] == sm).all() and (got_c[sample] == sc).all()
