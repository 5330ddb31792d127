"""CPU-side checks of template replacement (needle_template_parse, needle_replace_groups_lengths_packed_dev /
needle_replace_groups_fill_packed_dev): exported with the documented signatures; the parser against a hand-written table, against the
restated parser of replace_groups_cases on seeded random templates, and as a stand-alone program under -fsanitize=address,undefined;
every argument check of the device entries answers NEEDLE_ERR_INVALID with a message before any device call (also for an empty batch);
the Python surface and its ValueErrors.  And `splice_groups`, the reference every GPU test of the feature compares against, pinned to
hand-written answers.  None of this needs a GPU."""
import ctypes
import inspect
import os
import random
import re
import subprocess

import numpy as np
import pytest

from replace_groups_cases import FUZZ_REFUSED, FUZZ_REFUSED_CAP, expand, fuzz_chosen, parse, random_template, seeded_templates, splice_groups
from test_replace_abi import splice

NAMES = ("needle_template_parse", "needle_replace_groups_lengths_packed_dev", "needle_replace_groups_fill_packed_dev")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR = "error"

# (template, G, canonical form (groups, literals) or ERR)
TABLE = [
    ("$1", 1, ([1], ["", ""])),
    ("$0", 0, ([0], ["", ""])),
    ("$0", 5, ([0], ["", ""])),
    ("a$1b$2c", 2, ([1, 2], ["a", "b", "c"])),
    ("$12", 1, ([1], ["", "2"])),
    ("$12", 3, ([1], ["", "2"])),
    ("$12", 12, ([12], ["", ""])),
    ("$123", 12, ([12], ["", "3"])),
    ("$10", 9, ([1], ["", "0"])),
    ("$10", 10, ([10], ["", ""])),
    ("$00", 3, ([0], ["", ""])),      # 00 is still group 0
    ("$01", 3, ([1], ["", ""])),
    ("\\$1", 1, ([], ["$1"])),
    ("\\\\$1", 1, ([1], ["\\", ""])),
    ("\\a\\1", 0, ([], ["a1"])),
    ("$1$1", 1, ([1, 1], ["", "", ""])),
    ("", 0, ([], [""])),
    ("", 16, ([], [""])),
    ("plain {text}", 2, ([], ["plain {text}"])),
    ("$1" * 16, 1, ([1] * 16, [""] * 17)),
    ("$1" * 17, 1, ERR),
    ("x$1" * 16 + "x", 1, ([1] * 16, ["x"] * 17)),
    ("x" * 4096, 0, ([], ["x" * 4096])),
    ("x" * 4097, 0, ERR),
    ("x" * 4090 + "$1" + "y" * 6, 1, ([1], ["x" * 4090, "y" * 6])),
    ("x" * 4090 + "$1" + "y" * 7, 1, ERR),
    ("\\x" * 4096, 0, ([], ["x" * 4096])),
    ("\\x" * 4097, 0, ERR),
    ("ab\\", 1, ERR),
    ("\\", 0, ERR),
    ("ab$", 1, ERR),
    ("$", 0, ERR),
    ("$x", 1, ERR),
    ("$$1", 1, ERR),
    ("$ 1", 1, ERR),
    ("${a}", 1, ERR),
    ("${1}", 1, ERR),
    ("$4", 3, ERR),
    ("$1", 0, ERR),
    ("$9", 8, ERR),
    ("a\U0001f600$1\ud800", 1, ([1], ["a\U0001f600", "\ud800"])),  # a surrogate pair (two units) and a lone surrogate in literals
]


@pytest.fixture(scope="module")
def lib():
    from needle_amd import build
    build.build()
    from needle_amd import _lib
    return _lib.lib()


def u16(t):
    return np.frombuffer(t.encode("utf-16-le", "surrogatepass"), dtype=np.uint16) if isinstance(t, str) else np.asarray(t, np.uint16)


def lib_parse(lib, t, G):
    """needle_template_parse -> (groups, literals as lists of code units), or ERR with a non-empty message.  First the sizing call with
    NULL outputs, then the exact capacities."""
    from needle_amd import _lib
    u = np.ascontiguousarray(u16(t))
    k, nl = ctypes.c_uint32(77), ctypes.c_uint32(77)
    rc = lib.needle_template_parse(u.ctypes.data if u.size else None, u.size, G, None, 0, None, 0, None, 0, ctypes.byref(k), ctypes.byref(nl))
    if rc != _lib.NEEDLE_OK:
        assert rc == _lib.ERR_INVALID and lib.needle_last_error()
        return ERR
    groups, loff, lits = np.full(k.value + 1, -5, np.int32), np.full(k.value + 3, 9, np.uint32), np.full(nl.value + 1, 7, np.uint16)
    assert lib.needle_template_parse(u.ctypes.data if u.size else None, u.size, G, groups.ctypes.data, k.value, loff.ctypes.data, k.value + 2,
                                     lits.ctypes.data, nl.value, None, None) == _lib.NEEDLE_OK
    assert groups[-1] == -5 and loff[-1] == 9 and lits[-1] == 7  # nothing behind the capacities
    assert loff[0] == 0 and loff[k.value + 1] == nl.value and (np.diff(loff[:k.value + 2].astype(np.int64)) >= 0).all()
    return groups[:-1].tolist(), [lits[loff[i]:loff[i + 1]].tolist() for i in range(k.value + 1)]


def as_units(form):
    return form if form == ERR else (form[0], [u16(x).tolist() for x in form[1]])


def test_symbols_exported_with_the_documented_signatures(lib):
    from needle_amd import _lib
    header = open(os.path.join(ROOT, "include", "needle_hip.h")).read()
    squeeze = lambda s: re.sub(r"\s+", " ", s)
    flat = squeeze(header)
    for n in NAMES:
        assert hasattr(lib, n), n
        assert n in _lib.EXPORTS, n
    assert "#define NEEDLE_TEMPLATE_MAX_REFS 16" in header and _lib.TEMPLATE_MAX_REFS == 16
    assert squeeze("typedef struct { uint32_t n_refs; /* K */ const int32_t *groups; /* K group numbers, each in [0, n_planes) */ "
                   "const uint32_t *lit_offsets; /* K + 2, code units */ const void *lits; /* code units of the ROWS' char width */ } "
                   "needle_template;") in flat
    assert [f for f, _ in _lib.Template._fields_] == ["n_refs", "groups", "lit_offsets", "lits"]
    assert ctypes.sizeof(_lib.Template) == 32
    assert squeeze("int needle_template_parse(const uint16_t *tmpl, size_t n_units, uint32_t n_groups, int32_t *groups, uint32_t groups_cap, "
                   "uint32_t *lit_offsets, uint32_t lit_offsets_cap, uint16_t *lits, uint32_t lits_cap, uint32_t *n_refs, "
                   "uint32_t *n_lit_units);") in flat
    assert squeeze("int needle_replace_groups_lengths_packed_dev(const needle_packed_view *rows, const uint64_t *d_match_offsets, "
                   "const int32_t *d_group_start, const int32_t *d_group_end, uint64_t plane_stride, uint32_t n_planes, "
                   "const needle_template *tmpl, uint64_t *d_out_lengths, void *hip_stream);") in flat
    assert squeeze("int needle_replace_groups_fill_packed_dev(const needle_packed_view *rows, const uint64_t *d_match_offsets, "
                   "const int32_t *d_group_start, const int32_t *d_group_end, uint64_t plane_stride, uint32_t n_planes, "
                   "const needle_template *tmpl, const uint64_t *d_out_offsets, void *d_out_data, void *hip_stream);") in flat
    assert len(lib.needle_template_parse.argtypes) == 11
    assert len(lib.needle_replace_groups_lengths_packed_dev.argtypes) == 9
    assert len(lib.needle_replace_groups_fill_packed_dev.argtypes) == 10
    # the three places that listed the gap are gone
    assert "Out of scope: group references in replacements" not in header
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "`$1` in replacements (the planes are its input)" not in design and "group references (the group planes exist" not in design


def test_template_table(lib):
    for t, G, want in TABLE:
        assert parse(u16(t).tolist(), G) == as_units(want), ("restated", t[:40], G)
        assert lib_parse(lib, t, G) == as_units(want), ("library", t[:40], G)


def test_error_messages_name_position_and_rule(lib):
    for t, G, at, word in (("ab\\", 1, 2, "escapes"), ("ab$", 1, 2, "$"), ("a$x", 1, 1, "group number"), ("xy${a}", 1, 2, "named"),
                           ("..$4", 3, 2, "no group"), ("$1" * 17, 1, 32, "NEEDLE_TEMPLATE_MAX_REFS"), ("x" * 4097, 0, 4096, "NEEDLE_REPLACE_MAX_UNITS")):
        assert lib_parse(lib, t, G) == ERR
        msg = lib.needle_last_error().decode()
        assert "code unit %d:" % at in msg and word in msg, (t[:20], msg)
    assert lib_parse(lib, "$x", 1) == ERR and "named" not in lib.needle_last_error().decode()  # ${name} has a message of its own


def test_capacities(lib):
    from needle_amd import _lib
    u = np.ascontiguousarray(u16("a$1b$2c"))
    g, lo, li = np.zeros(2, np.int32), np.zeros(4, np.uint32), np.zeros(3, np.uint16)
    call = lambda gc, oc, lc, gp=True: lib.needle_template_parse(u.ctypes.data, u.size, 2, g.ctypes.data if gp else None, gc, lo.ctypes.data, oc,
                                                                 li.ctypes.data, lc, None, None)
    assert call(2, 4, 3) == _lib.NEEDLE_OK and g.tolist() == [1, 2] and lo.tolist() == [0, 1, 2, 3] and li.tolist() == [97, 98, 99]
    for caps in ((1, 4, 3), (2, 3, 3), (2, 4, 2)):
        assert call(*caps) == _lib.ERR_INVALID and lib.needle_last_error()
    assert call(2, 4, 3, gp=False) == _lib.ERR_INVALID  # NULL with a capacity
    assert lib.needle_template_parse(None, 3, 2, None, 0, None, 0, None, 0, None, None) == _lib.ERR_INVALID  # NULL template with units
    assert lib.needle_template_parse(None, 0, 2, None, 0, None, 0, None, 0, None, None) == _lib.NEEDLE_OK


def test_random_templates(lib):
    """2000 seeded templates over `$\\{}019ab` at each G: the library's parser is the restated one."""
    errors = parsed = 0
    for G in (0, 1, 9, 10, 16):
        rng = random.Random(1000 + G)
        for _ in range(2000):
            t = random_template(rng)
            want = parse(t, G)
            assert lib_parse(lib, t, G) == want, (t, G)
            errors += want == ERR
            parsed += want != ERR and len(want[0]) > 0
    assert errors > 2000 and parsed > 500


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("template") / "template_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "c", "template_check.cpp"), "-o", exe])

    def run(cases):
        text = "".join("%d %d %s\n" % (G, len(u), " ".join(str(int(x)) for x in u)) for u, G in cases)
        r = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr[-4000:]
        lines = r.stdout.split("\n")[:-1]
        assert len(lines) == len(cases)
        out = []
        for ln in lines:
            if ln == "E":
                out.append(ERR)
                continue
            x = [int(v) for v in ln.split()]
            k = x[0]
            off, lits = x[1 + k:3 + 2 * k], x[3 + 2 * k:]
            out.append((x[1:1 + k], [lits[off[i]:off[i + 1]] for i in range(k + 1)]))
        return out
    return run


def test_parser_header_stand_alone_under_sanitizers(program):
    rng = random.Random(5)
    cases = [(u16(t).tolist(), G) for t, G, _ in TABLE] + [(u16(random_template(rng, max_len=12)).tolist(), G) for G in (0, 1, 9, 10, 16) for _ in range(200)]
    want = [as_units(w) for _, _, w in TABLE] + [parse(u, G) for u, G in cases[len(TABLE):]]
    assert program(cases) == want


# ---- the device entries' argument checks.  Host buffers stand in for device pointers: the calls must refuse before any is dereferenced
_data = np.zeros(64, dtype=np.uint8)
_offsets = np.array([0, 3, 7], dtype=np.uint64)
_moff = np.zeros(3, dtype=np.uint64)
_gs = np.zeros(8, dtype=np.int32)
_ge = np.zeros(8, dtype=np.int32)
_lens = np.zeros(2, dtype=np.uint64)
_ooff = np.zeros(3, dtype=np.uint64)
_out = np.zeros(64, dtype=np.uint8)
_lits = np.zeros(8192, dtype=np.uint8)


def _view(data_ptr=None, cw=1, n=2, offsets_ptr=None):
    from needle_amd import _lib
    v = _lib.PackedView()
    v.data = _data.ctypes.data if data_ptr is None else data_ptr
    v.char_width, v.n_rows = cw, n
    v.offsets = _offsets.ctypes.data if offsets_ptr is None else offsets_ptr
    return v


def _tmpl(groups=(1, 2), loff=(0, 1, 2, 3), n_refs=None, lits=True, null=False, groups_null=False, loff_null=False):
    """-> (needle_template or None, the arrays it points into)"""
    from needle_amd import _lib
    if null:
        return None, ()
    g, lo = np.asarray(groups, np.int32), np.asarray(loff, np.uint32)
    t = _lib.Template()
    t.n_refs = len(groups) if n_refs is None else n_refs
    t.groups = None if groups_null or not g.size else g.ctypes.data
    t.lit_offsets = None if loff_null else lo.ctypes.data
    t.lits = _lits.ctypes.data if lits else None
    return t, (g, lo)


def _lengths(lib, v, moff=True, planes=3, out=True, **kw):
    t, keep = _tmpl(**kw)
    return lib.needle_replace_groups_lengths_packed_dev(ctypes.byref(v) if v is not None else None, _moff.ctypes.data if moff else None, _gs.ctypes.data,
                                                        _ge.ctypes.data, 2, planes, ctypes.byref(t) if t is not None else None,
                                                        _lens.ctypes.data if out else None, None)


def _fill(lib, v, moff=True, planes=3, ooff=True, out=True, out_ptr=None, **kw):
    t, keep = _tmpl(**kw)
    outp = (_out.ctypes.data if out_ptr is None else out_ptr) if out else None
    return lib.needle_replace_groups_fill_packed_dev(ctypes.byref(v) if v is not None else None, _moff.ctypes.data if moff else None, _gs.ctypes.data,
                                                     _ge.ctypes.data, 2, planes, ctypes.byref(t) if t is not None else None,
                                                     _ooff.ctypes.data if ooff else None, outp, None)


def _refused(lib, rc, what):
    from needle_amd import _lib
    assert rc == _lib.ERR_INVALID, what
    assert lib.needle_last_error(), what


BAD_TEMPLATES = [
    ("NULL template", dict(null=True)),
    ("NULL literal offsets", dict(loff_null=True)),
    ("NULL groups with references", dict(groups_null=True)),
    ("17 references", dict(groups=[1] * 17, loff=[0] * 19)),
    ("n_refs 17 alone", dict(n_refs=17)),
    ("a group that is no plane", dict(groups=(1, 3))),
    ("a negative group", dict(groups=(-1, 2))),
    ("n_planes 0", dict(planes=0, groups=(), loff=(0, 1))),
    ("offsets[0] != 0", dict(loff=(1, 1, 2, 3))),
    ("a decreasing pair", dict(loff=(0, 5, 4, 9))),
    ("a total above the limit", dict(loff=(0, 4000, 4000, 4097))),
]


def test_validation_without_device(lib):
    bad_views = [None, _view(offsets_ptr=0), _view(cw=0), _view(cw=3), _view(cw=4), _view(data_ptr=_data.ctypes.data + 1),
                 _view(data_ptr=_data.ctypes.data + 2, cw=2)]
    for i, v in enumerate(bad_views):
        _refused(lib, _lengths(lib, v), ("lengths, view", i))
        _refused(lib, _fill(lib, v), ("fill, view", i))
    for n in (2, 0):  # every refusal also with an empty batch: the arguments are checked first
        _refused(lib, _lengths(lib, _view(n=n), moff=False), ("lengths: NULL match offsets", n))
        _refused(lib, _lengths(lib, _view(n=n), out=False), ("lengths: NULL output", n))
        _refused(lib, _fill(lib, _view(n=n), moff=False), ("fill: NULL match offsets", n))
        _refused(lib, _fill(lib, _view(n=n), ooff=False), ("fill: NULL output offsets", n))
        _refused(lib, _fill(lib, _view(n=n), out=False), ("fill: NULL output", n))
        _refused(lib, _fill(lib, _view(n=n), out_ptr=_out.ctypes.data + 2), ("fill: output not 4-byte aligned", n))
        _refused(lib, _fill(lib, _view(n=n), lits=False), ("fill: NULL literals with units", n))
        for what, kw in BAD_TEMPLATES:
            _refused(lib, _lengths(lib, _view(n=n), **kw), ("lengths", what, n))
            _refused(lib, _fill(lib, _view(n=n), **kw), ("fill", what, n))


def test_empty_batch_is_ok_and_the_limits(lib):
    from needle_amd import _lib
    for cw in (1, 2):
        for kw in (dict(groups=(), loff=(0, 0)), dict(groups=(), loff=(0, 4096)), dict(groups=(0,), loff=(0, 0, 0)), dict(groups=(2, 2), loff=(0, 0, 7, 7)),
                   dict(groups=[2] * 16, loff=[0] * 18), dict(groups=[0] * 16, loff=list(range(0, 4097, 256)) + [4096])):
            assert _lengths(lib, _view(cw=cw, n=0), **kw) == _lib.NEEDLE_OK, kw
            assert _fill(lib, _view(cw=cw, n=0), **kw) == _lib.NEEDLE_OK, kw
        assert _lengths(lib, _view(cw=cw, n=0), lits=False) == _lib.NEEDLE_OK            # the lengths entry never reads the units
        assert _fill(lib, _view(cw=cw, n=0), lits=False, loff=(0, 0, 0, 0)) == _lib.NEEDLE_OK  # empty literals need no units
        assert _fill(lib, _view(cw=cw, n=0), planes=1, groups=(0, 0)) == _lib.NEEDLE_OK


def test_fuzz_refusals_counted_on_the_cpu(lib):
    """The patterns the device fuzz (test_gpu_replace_groups.py) leaves out: those of its 200 whose captures are refused.  Needs no
    device; the count is pinned, the cap is 1 %, and every seeded template of the others parses."""
    from needle_amd.pattern import DFACompiler
    chosen = fuzz_chosen()
    assert len(chosen) == 200 and FUZZ_REFUSED_CAP * 100 <= 1 * len(chosen)
    refused = 0
    for i, regex in chosen:
        p = DFACompiler.compile(regex, "f")
        if not p.captures_info()["available"]:
            refused += 1
            continue
        for t in seeded_templates(i, p.group_count(), 3):
            groups, literals = p.parse_template(t)
            assert (groups, [[ord(c) for c in x] for x in literals]) == parse(t, p.group_count())
    assert refused == FUZZ_REFUSED <= FUZZ_REFUSED_CAP


# ---- the reference of the GPU tests
def test_reference_splice_groups():
    row = "ab 10-20 cd 3-4"
    swap = ([2, 1], ["", "-", ""])
    m1, m2 = [(3, 8), (3, 5), (6, 8)], [(12, 15), (12, 13), (14, 15)]
    assert splice_groups(row, [m1, m2], *swap) == "ab 20-10 cd 4-3"
    assert splice_groups(row, [[(-1, -1), (-1, -1), (-1, -1)], m2], *swap) == "ab 10-20 cd 4-3"              # a kept match is no piece
    assert splice_groups(row, [m1, [(-1, 9), (12, 13), (14, 15)]], *swap) == "ab 20-10 cd 3-4"               # ... whatever its other values
    assert splice_groups(row, [[(3, 8), (-1, -1), (6, 8)], m2], [1, 2], ["[", "|", "]"]) == "ab [|20] cd [3|4]"  # a group not passed
    assert splice_groups(row, [[(3, 8), (-1, 5), (6, 8)]], [1, 2], ["[", "|", "]"]) == "ab [|20] cd 3-4"     # (only its start decides)
    # planes that leave the row or are reversed: the clamps
    assert splice_groups("abcdef", [[(2, 99), (4, 2), (-0, 99)]], [1, 2], ["<", "|", ">"]) == "ab<|abcdef>"
    assert splice_groups("abcdef", [[(4, 1), (3, 5), (99, 100)]], [1, 2], ["<", "|", ">"]) == "abcd<de|>ef"   # e' = s': nothing removed
    assert splice_groups("abcdef", [[(0, 6), (5, 6), (0, 1)]], [1, 2, 1], ["", "", "", ""]) == "faf"          # a group text from anywhere, twice
    # $0 is the identity
    for planes in ([m1, m2], [m1], []):
        assert splice_groups(row, planes, [0], ["", ""]) == row
    # no references: the plain splice
    for r, matches in (("abc123def45", [(3, 6), (9, 11)]), ("aabbcc", [(0, 2), (2, 4), (4, 6)]), ("", []), ("x", [(0, 1)]), ("ab", [(0, 1), (1, 1)])):
        for repl in ("", "#", "<number>"):
            assert splice_groups(r, [[m] for m in matches], [], [repl]) == splice(r, matches, repl)
    got = splice_groups(np.array([1, 2, 3, 4, 5], np.uint16), [[(1, 4), (3, 4), (1, 2)]], [1, 2], [np.array([9], np.uint16), np.zeros(0, np.uint16), np.array([8, 8], np.uint16)])
    assert got.dtype == np.uint16 and got.tolist() == [1, 9, 4, 2, 8, 8, 5]
    assert expand([1, 1], ["<", "|", ">"], "hello", [(0, 5), (1, 3)]) == "<el|el>"
    assert expand([1], ["a", "b"], "hello", [(0, 5), None]) == "ab"


def test_python_surface(lib):
    from needle_amd.pattern import DFACompiler, Pattern, PatternException
    assert list(inspect.signature(Pattern.splice_groups_packed).parameters) == [
        "data", "offsets", "match_offsets", "gstart", "gend", "groups", "literals", "stream", "out", "out_start"]
    assert isinstance(inspect.getattr_static(Pattern, "splice_groups_packed"), staticmethod)
    for name in ("replace_all_groups_packed", "replace_first_groups_packed"):
        assert list(inspect.signature(getattr(Pattern, name)).parameters) == ["self", "data", "offsets", "repl", "stream", "out", "out_start"]
    assert list(inspect.signature(Pattern.replace_all_groups_strings).parameters) == ["self", "strings", "repl"]
    assert list(inspect.signature(Pattern.replace_all_groups_bytes).parameters) == ["self", "rows", "repl"]
    p = DFACompiler.compile(r"([0-9]+)-([0-9]+)")
    assert p.parse_template("$2-$1") == ([2, 1], ["", "-", ""])
    assert p.parse_template("$12\\$ λ\U0001f600") == ([1], ["", "2$ λ\U0001f600"])
    assert p.parse_template("") == ([], [""])
    assert DFACompiler.compile("[a-c]+").parse_template("x$0y") == ([0], ["x", "y"])
    for bad, word in (("$3", "no group"), ("${a}", "named"), ("$", "$"), ("a\\", "escapes"), ("$1" * 17, "MAX_REFS")):
        with pytest.raises(ValueError, match=re.escape(word)):
            p.parse_template(bad)
    # the template as the device entries take it
    t, (g, loff, units) = Pattern._template([2, 1], ["", "-", "é"], 1, 3)
    assert t.n_refs == 2 and g.tolist() == [2, 1] and loff.tolist() == [0, 0, 1, 2] and units.dtype == np.uint8 and units.tolist() == [45, 233]
    t, (g, loff, units) = Pattern._template([], ["λ猫"], 2, 1)
    assert t.n_refs == 0 and t.groups is None and loff.tolist() == [0, 2] and units.dtype == np.uint16
    for groups, literals, cw, planes in (([1], ["a"], 1, 2), ([1] * 17, [""] * 18, 1, 2), ([2], ["", ""], 1, 2), ([-1], ["", ""], 1, 2),
                                         ([1], ["λ", ""], 1, 2), ([1], ["x" * 4096, "y"], 2, 2)):
        with pytest.raises(ValueError):
            Pattern._template(groups, literals, cw, planes)
    # a pattern whose captures are refused: the reason, before anything is packed or sent
    with pytest.raises(PatternException, match="NULLABLE_LOOP"):
        DFACompiler.compile(r"(a*)+").replace_all_groups_strings(["aab"], "$1")
    with pytest.raises(PatternException, match="NULLABLE_LOOP"):
        DFACompiler.compile(r"(a*)+").replace_all_groups_bytes([b"aab"], "$1")
