"""bindings/jni/needle_jni.c on the CPU, without a JDK and without a JVM: compiled against the stand-in tests/jni/jni.h (NOT a JVM's table
layout -- nothing built here is ever loaded by one) together with the fake JNIEnv tests/jni/fake_jvm.c, which hands out COPIES of arrays
between sentinels and records what a shim must never do.

- the shim compiles without a warning and exports exactly the natives Native.java declares;
- a SIGNATURE CHECK: every `static native` of Native.java against the C definition of its symbol in the preprocessed shim (return type,
  parameter types, order, count), and every Native.<name>(...) call of bindings/java against the declarations.  The Java sources remain
  uncompiled: this is a comparison of texts;
- the device-free natives through the fake env against the ctypes path of needle_amd/_lib.py;
- argument validation of every native that takes an array or a buffer;
- both again in tests/c/jni_shim_check.c under AddressSanitizer and UBSan (a stand-alone program; no Python process loads sanitized code).
The scan natives' results are tests/test_gpu_jni_shim.py's."""
import os
import re
import subprocess

import pytest

import jni_shim_cases as J
from conftest import ROOT


@pytest.fixture(scope="module")
def built(tmp_path_factory):
    return J.build_fake(tmp_path_factory.mktemp("jni_fake"))


@pytest.fixture(scope="module")
def fake(built):
    f = J.Fake(built[0])
    yield f
    f.reset()


def test_shim_compiles_without_warnings_and_exports_the_declared_natives(built):
    """gcc -std=c99 -Wall -Wextra -Werror -Wno-unused-parameter; `nm -D`: the Java_* symbols are exactly those computed from Native.java."""
    so, diagnostics = built
    assert diagnostics.strip() == "", diagnostics
    out = subprocess.run(["nm", "-D", "--defined-only", so], capture_output=True, text=True, check=True).stdout
    exported = sorted(ln.split()[-1] for ln in out.splitlines() if ln.split()[-1].startswith("Java_"))
    declared = sorted(d["symbol"] for d in J.java_natives())
    assert len(set(declared)) == len(declared), "two declarations share one symbol"
    assert exported == declared, (sorted(set(exported) - set(declared)), sorted(set(declared) - set(exported)))


def c_definitions():
    """{symbol: (return type, [parameter types])} from the preprocessed shim (NATIVE and BOOL_CALL expanded)."""
    cmd = ["gcc", "-E", "-P", "-std=c99", "-I", J.JNI_DIR, "-I", os.path.join(ROOT, "include"), J.SHIM]
    text = subprocess.run(cmd, capture_output=True, text=True, check=True).stdout
    text = re.sub(r"__attribute__\s*\(\((?:[^()]|\([^()]*\))*\)\)", " ", text)
    defs = {}
    for m in re.finditer(r"([A-Za-z_][\w \t\*]*?)\s*\b(Java_\w+)\s*\(([^)]*)\)\s*\{", text):
        ret, symbol = " ".join(m.group(1).split()), m.group(2)
        params = []
        for p in m.group(3).split(","):
            t = re.sub(r"\b\w+\s*$", "", p.strip())  # drop the parameter's name
            params.append(re.sub(r"\s*\*\s*", " *", " ".join(t.split())))
        assert symbol not in defs, "defined twice: " + symbol
        defs[symbol] = (ret, params)
    return defs


def test_signatures_of_native_java_match_the_c_definitions():
    """A signature check (texts only): each declaration pairs with exactly one definition, nothing is left over on either side."""
    decls, defs = J.java_natives(), c_definitions()
    assert len(decls) >= 45
    by_symbol = {d["symbol"]: d for d in decls}
    assert len(by_symbol) == len(decls)
    assert sorted(by_symbol) == sorted(defs), (sorted(set(defs) - set(by_symbol)), sorted(set(by_symbol) - set(defs)))
    names = [d["name"] for d in decls]
    assert len(set(names)) == len(names), "an overloaded native: it would need the long mangled symbol, written by hand"
    for symbol, d in by_symbol.items():
        ret, params = defs[symbol]
        assert ret == d["c_ret"], (d["name"], "returns", ret, "declared", d["ret"])
        assert params == d["c_params"], (d["name"], params, d["c_params"])


def java_calls():
    """(file, name, number of arguments) of every Native.<name>( call under bindings/java (comments stripped, parentheses balanced)."""
    calls = []
    for dirpath, _, files in os.walk(J.JAVA_DIR):
        for f in files:
            if not f.endswith(".java"):
                continue
            text = J.strip_java_comments(open(os.path.join(dirpath, f)).read())
            for m in re.finditer(r"\bNative\.(\w+)\s*\(", text):
                depth, i, commas, empty, in_str = 1, m.end(), 0, True, False
                while depth:
                    ch = text[i]
                    if in_str:
                        if ch == "\\":
                            i += 1
                        elif ch == '"':
                            in_str = False
                    elif ch == '"':
                        in_str, empty = True, False
                    elif ch in "([{":
                        depth, empty = depth + 1, False
                    elif ch in ")]}":
                        depth -= 1
                    elif ch == "," and depth == 1:
                        commas += 1
                    elif not ch.isspace():
                        empty = False
                    i += 1
                calls.append((f, m.group(1), 0 if empty else commas + 1))
    return calls


def test_java_callers_name_declared_natives_with_a_declared_argument_count():
    """Textually: every Native.<name>(...) of bindings/java names a declared native, with as many arguments as one of its declarations."""
    arity = {}
    for d in J.java_natives():
        arity.setdefault(d["name"], set()).add(len(d["params"]))
    calls = java_calls()
    assert len(calls) >= 50
    for f, name, n in calls:
        assert name in arity, (f, name, "is not declared in Native.java")
        assert n in arity[name], (f, name, n, "arguments; declared with", sorted(arity[name]))
    assert {"findPacked16PackedHost", "findPacked8PackedHost", "findPacked16Host", "findPacked8Host"} <= {c[1] for c in calls}


def test_every_native_with_an_array_or_buffer_has_validation_cases():
    """The table of validation cases names EVERY native that takes an array or a buffer, with as many arguments as it is declared with and
    an array wherever the declaration has one."""
    for d in J.java_natives():
        takes = [i for i, (t, _) in enumerate(d["params"]) if t.endswith("]") or t.endswith("ByteBuffer")]
        if not takes:
            assert d["name"] not in J.VALIDATION
            continue
        if d["name"] in J.VALIDATION_BY_HAND:
            continue
        assert d["name"] in J.VALIDATION, d["name"]
        spec = J.VALIDATION[d["name"]][0]
        assert len(spec) == len(d["params"]), d["name"]
        assert [i for i, a in enumerate(spec) if a[0] in ("a", "b", "offsets")] == takes, d["name"]
        for i in takes:
            t, a = d["params"][i][0], spec[i]
            assert (a[0] == "b") == t.endswith("ByteBuffer") and (a[0] != "a" or a[1] + "[]" == t) and (a[0] != "offsets" or t == "long[]"), (d["name"], i)


def test_device_free_natives_against_ctypes(fake):
    """compile (code units >= 0x8000 among them), lastError, serialize, deserialize, fromTables, tuningInfo, prefilterInfo, prefilterState,
    setPrefilter, utf16Route, findAllPackedFilter, trimScratch, setCreate (0, 1, 3, 32, 33 patterns) / setDestroy: each equal to what the same
    library gives through ctypes for the same input; after every call no pin is outstanding and the fault log is empty."""
    J.run_ops(fake, J.device_free_ops())
    assert fake.L.fj_get_calls() > 0
    fake.reset()


def test_from_tables_of_a_compiled_pattern_gives_its_tables_back():
    """fromTables' reference in the test above is needle_pattern_from_tables on the same tables (the blob of a from-tables pattern is NOT
    the compiled pattern's: the compiler records more than the four tables).  Here that reference itself: the four tables of a compiled
    pattern, read through the accessors, give a pattern with the same class map and tables."""
    import numpy as np
    for regex in J.GOOD_REGEXES:
        rc, h, _ = J.lib_compile(regex)
        tb = J.lib_tables(h)
        rc2, h2 = J.lib_from_tables(tb)
        assert rc == 0 and rc2 == 0
        tb2 = J.lib_tables(h2)
        assert (tb["cm"] == tb2["cm"]).all() and tb["stride"] == tb2["stride"] and tb["fixed_len"] == tb2["fixed_len"]
        assert (tb["ns"] == tb2["ns"]).all() and (tb["mc"] == tb2["mc"]).all()
        assert all(np.array_equal(a, b) for a, b in zip(tb["tables"] + tb["accepting"], tb2["tables"] + tb2["accepting"]))


def test_argument_validation_of_every_native(fake):
    """Each required argument null in turn, each array one element short of the header's contract, empty offsets, a heap ByteBuffer, and
    Get<T>ArrayElements returning NULL at every position: NEEDLE_ERR_INVALID (null where a String or byte[] is returned), no outstanding
    pin, an empty fault log, every array byte-identical.  No case reaches a scan entry of the library, so none needs a GPU."""
    ops = J.validation_ops()
    assert sum(1 for op in ops if op[0] == "label") >= 300
    J.run_ops(fake, ops)
    fake.reset()


def test_validation_table_counts_every_get_of_a_valid_call(fake):
    """The positions at which the test above makes Get<T>ArrayElements return NULL come from a hand-written count per native.  One valid
    call of each native, with every Get beyond that count ordered to return NULL: exactly that many are made and no NULL is handed out,
    so no position of any native is left untried.  (Without a device the scan entries answer NEEDLE_ERR_DEVICE; the status is not what
    this test is about.)"""
    ops = J.validation_ops(get_counts=True)
    assert sum(1 for op in ops if op[0] == "gets_exact") == len(J.VALIDATION) + 2
    J.run_ops(fake, ops)
    fake.reset()


def test_the_fake_jvm_records_what_it_should(fake):
    """The fake itself: copies, modes, sentinels, foreign and double releases, regions, nulls -- so that an empty fault log means something."""
    import ctypes
    import numpy as np
    L, env = fake.L, fake.env
    fn = ctypes.cast(env, ctypes.POINTER(ctypes.POINTER(ctypes.c_void_p)))[0]  # the table, in tests/jni/jni.h's order
    VP, I = ctypes.c_void_p, ctypes.c_int32
    get_int = ctypes.CFUNCTYPE(VP, VP, VP, VP)(fn[9])
    get_long = ctypes.CFUNCTYPE(VP, VP, VP, VP)(fn[10])
    rel_int = ctypes.CFUNCTYPE(None, VP, VP, VP, I)(fn[14])
    rel_long = ctypes.CFUNCTYPE(None, VP, VP, VP, I)(fn[15])
    set_int = ctypes.CFUNCTYPE(None, VP, VP, I, I, VP)(fn[16])
    get_len = ctypes.CFUNCTYPE(I, VP, VP)(fn[1])
    direct = ctypes.CFUNCTYPE(VP, VP, VP)(fn[4])
    check = ctypes.CFUNCTYPE(ctypes.c_ubyte, VP)(fn[2])
    fake.reset()
    a, b = fake.array("int", [1, 2, 3]), fake.array("int", [7, 7, 7])
    is_copy = ctypes.c_ubyte(0)
    p = get_int(env, a, ctypes.byref(is_copy))
    assert is_copy.value == 1 and p != L.fj_array_data(a) and fake.pins() == 1
    view = (ctypes.c_int32 * 3).from_address(p)
    view[0] = 10
    assert fake.read(a).tolist() == [1, 2, 3]           # a copy: nothing reaches the array before a release
    rel_int(env, a, p, 1)                                # JNI_COMMIT: copied back, still outstanding
    assert fake.read(a).tolist() == [10, 2, 3] and fake.pins() == 1
    view[1] = 20
    rel_int(env, a, p, 2)                                # JNI_ABORT: freed without copying back
    assert fake.read(a).tolist() == [10, 2, 3] and fake.pins() == 0 and fake.faults() == ""
    rel_int(env, a, p, 0)
    assert L.fj_fault_count(2) == 1, fake.faults()       # a second release
    p = get_int(env, a, None)
    rel_int(env, b, p, 0)
    rel_long(env, a, p, 0)
    assert L.fj_fault_count(1) == 2 and fake.pins() == 1  # another array, another element type
    (ctypes.c_int32 * 1).from_address(p + 12)[0] = 5      # one element past the copy
    rel_int(env, a, p, 0)
    assert L.fj_fault_count(6) == 1 and fake.pins() == 0
    q = get_int(env, a, None)
    (ctypes.c_int32 * 1).from_address(q - 4)[0] = 5       # one element in front of it
    rel_int(env, a, q, 2)
    assert L.fj_fault_count(6) == 2
    junk = np.zeros(4, dtype=np.int32)
    rel_int(env, a, junk.ctypes.data, 0)
    assert L.fj_fault_count(0) == 1                        # a pointer never handed out
    assert check(env) == 0
    set_int(env, a, 2, 2, junk.ctypes.data)
    assert L.fj_fault_count(3) == 1 and check(env) == 1 and fake.read(a).tolist() == [10, 2, 3]
    L.fj_clear_exception()
    assert get_len(env, None) == 0 and get_int(env, None, None) is None and L.fj_fault_count(4) == 2
    assert get_long(env, a, None) is None and L.fj_fault_count(7) == 1   # GetLongArrayElements of an int[]
    assert direct(env, a) is None and L.fj_fault_count(5) == 1            # no buffer at all
    assert direct(env, fake.heap_buffer()) is None and L.fj_fault_count(5) == 1  # a heap buffer: NULL, as specified, and no fault
    mem = np.arange(8, dtype=np.uint8)
    assert direct(env, fake.buffer(mem)) == mem.ctypes.data
    L.fj_fail_gets(1, 1)
    p1 = get_int(env, a, None)
    assert p1 and get_int(env, a, None) is None and check(env) == 1 and L.fj_fail_gets_left() == 0
    rel_int(env, a, p1, 0)
    assert "double_release=1" in fake.faults() and "last:" in fake.faults()
    fake.reset()
    assert fake.faults() == "" and fake.pins() == 0 and L.fj_exception_pending() == 0


def test_device_free_and_validation_cases_under_sanitizers(tmp_path):
    """tests/c/jni_shim_check.c: the shim and the fake JVM with -fsanitize=address,undefined -fno-sanitize-recover=all (libneedle_hip.so as
    built), the two scripts above on its stdin; exit status 0."""
    (tmp_path / "jni_shim_dispatch.inc").write_text(J.dispatch_source())
    exe = str(tmp_path / "jni_shim_check")
    cmd = J.compile_command(exe, ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", str(tmp_path)],
                            sources=[os.path.join(ROOT, "tests", "c", "jni_shim_check.c"), J.SHIM, os.path.join(J.JNI_DIR, "fake_jvm.c")])
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-6000:]
    ops = J.device_free_ops() + J.validation_ops()
    r = subprocess.run([exe], input=J.ops_text(ops), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-500:], r.stderr[-6000:])
    assert "jni shim check ok: %d ops" % len(ops) in r.stdout
