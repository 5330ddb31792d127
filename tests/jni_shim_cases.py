"""What tests/test_jni_shim.py (CPU), tests/test_gpu_jni_shim.py (GPU) and tests/c/jni_shim_check.c (the sanitizer program) share:

- build_fake(): bindings/jni/needle_jni.c + tests/jni/fake_jvm.c against the stand-in tests/jni/jni.h as one libneedle_jni_fake.so;
- java_natives(): the `static native` declarations of Native.java, with the JNI symbol and the JNI types of each;
- Fake: that library through ctypes -- Java arrays, object arrays and direct buffers as the fake JVM's objects, natives by name;
- a tiny script language (`ops`) in which the device-free calls and the argument-validation cases are written ONCE: run_ops()
  runs a script on a Fake in this process, ops_text() writes it for the sanitizer program's stdin.

The stand-in header's table layout is not a JVM's: nothing built here is ever loaded by one.  The Java sources stay uncompiled; what
is checked of them is their text."""
import ctypes
import os
import re
import subprocess

import numpy as np

from conftest import ROOT

JNI_DIR = os.path.join(ROOT, "tests", "jni")
SHIM = os.path.join(ROOT, "bindings", "jni", "needle_jni.c")
JAVA_DIR = os.path.join(ROOT, "bindings", "java")
NATIVE_JAVA = os.path.join(JAVA_DIR, "com", "justinblank", "strings", "gpu", "Native.java")
SYMBOL_PREFIX = "Java_com_justinblank_strings_gpu_Native_"
CFLAGS = ["-std=c99", "-Wall", "-Wextra", "-Werror", "-Wno-unused-parameter"]
ERR_INVALID = 1

# Java type -> (JNI type in the C definition, letter of the JNI signature used in the long mangled name)
JNI_TYPES = {
    "void": ("void", "V"), "int": ("jint", "I"), "long": ("jlong", "J"), "float": ("jfloat", "F"), "boolean": ("jboolean", "Z"),
    "String": ("jstring", "Ljava/lang/String;"), "java.nio.ByteBuffer": ("jobject", "Ljava/nio/ByteBuffer;"), "ByteBuffer": ("jobject", "Ljava/nio/ByteBuffer;"),
    "byte[]": ("jbyteArray", "[B"), "char[]": ("jcharArray", "[C"), "short[]": ("jshortArray", "[S"), "int[]": ("jintArray", "[I"),
    "long[]": ("jlongArray", "[J"), "float[]": ("jfloatArray", "[F"), "short[][]": ("jobjectArray", "[[S"), "byte[][]": ("jobjectArray", "[[B"),
}


def mangle(s):
    """JNI name mangling of a name or a signature."""
    out = []
    for ch in s:
        if ch.isascii() and ch.isalnum():
            out.append(ch)
        else:
            out.append({"/": "_", "_": "_1", ";": "_2", "[": "_3"}.get(ch) or "_0%04x" % ord(ch))
    return "".join(out)


def strip_java_comments(text):
    text = re.sub(r"/\*.*?\*/", lambda m: re.sub(r"[^\n]", " ", m.group(0)), text, flags=re.S)
    return re.sub(r"//[^\n]*", "", text)


def java_natives():
    """[{name, ret, params: [(java type, name)], symbol, c_ret, c_params}] for every `static native` of Native.java; an overloaded name
    gets the long mangled symbol, every other the short one."""
    text = strip_java_comments(open(NATIVE_JAVA).read())
    decls = []
    for m in re.finditer(r"static\s+native\s+([\w.\[\]]+)\s+(\w+)\s*\(([^)]*)\)\s*;", text):
        params = []
        for p in [p.strip() for p in m.group(3).split(",") if p.strip()]:
            t, n = p.rsplit(None, 1)
            params.append((re.sub(r"\s+", "", t), n))
        decls.append({"name": m.group(2), "ret": m.group(1), "params": params})
    assert len(decls) == len(re.findall(r"\bnative\b", text)), "a `native` declaration the parser did not understand"
    names = [d["name"] for d in decls]
    for d in decls:
        d["symbol"] = SYMBOL_PREFIX + mangle(d["name"])
        if names.count(d["name"]) > 1:
            d["symbol"] += "__" + mangle("".join(JNI_TYPES[t][1] for t, _ in d["params"]))
        d["c_ret"] = JNI_TYPES[d["ret"]][0]
        d["c_params"] = ["JNIEnv *", "jclass"] + [JNI_TYPES[t][0] for t, _ in d["params"]]
    return decls


def compile_command(out, extra=(), sources=None):
    from needle_amd import build
    libdir = os.path.dirname(build.build())
    return (["gcc"] + CFLAGS + list(extra) + ["-I", JNI_DIR, "-I", os.path.join(ROOT, "include")] +
            (sources or [SHIM, os.path.join(JNI_DIR, "fake_jvm.c")]) + ["-L", libdir, "-lneedle_hip", "-Wl,-rpath," + libdir, "-o", out])


def build_fake(directory):
    """-> (path of libneedle_jni_fake.so, the compiler's output)."""
    so = os.path.join(str(directory), "libneedle_jni_fake.so")
    r = subprocess.run(compile_command(so, ["-O1", "-g", "-fPIC", "-shared"]), capture_output=True, text=True)
    assert r.returncode == 0, "the shim does not compile against tests/jni/jni.h:\n" + r.stderr[-6000:]
    return so, r.stderr


KINDS = {"byte": (1, np.int8), "char": (2, np.uint16), "short": (3, np.int16), "int": (4, np.int32), "long": (5, np.int64), "float": (6, np.float32)}
_CT = {"jint": ctypes.c_int32, "jlong": ctypes.c_int64, "jfloat": ctypes.c_float, "void": None}


class Fake:
    """libneedle_jni_fake.so through ctypes.  Objects of the fake JVM are plain integers (addresses) here; None is Java's null."""

    def __init__(self, so):
        from needle_amd import _lib
        _lib.lib()  # first: one libneedle_hip.so (and one HIP runtime, torch's) serves this process
        L = self.L = ctypes.CDLL(so)
        VP = ctypes.c_void_p
        for name, res, args in (("fj_env", VP, []), ("fj_new_array", VP, [ctypes.c_int, ctypes.c_int32, VP]), ("fj_new_object_array", VP, [ctypes.c_int32, VP]),
                                ("fj_new_direct_buffer", VP, [VP, ctypes.c_int64]), ("fj_new_heap_buffer", VP, []), ("fj_array_length", ctypes.c_int32, [VP]),
                                ("fj_array_bytes", ctypes.c_size_t, [VP]), ("fj_array_data", VP, [VP]), ("fj_string_utf", ctypes.c_char_p, [VP]),
                                ("fj_outstanding_pins", ctypes.c_int, []), ("fj_fault_count", ctypes.c_int, [ctypes.c_int]), ("fj_fault_log", ctypes.c_char_p, []),
                                ("fj_exception_pending", ctypes.c_int, []), ("fj_clear_exception", None, []), ("fj_fail_gets", None, [ctypes.c_int, ctypes.c_int]),
                                ("fj_fail_gets_left", ctypes.c_int, []), ("fj_get_calls", ctypes.c_int, []), ("fj_reset", None, [])):
            f = getattr(L, name)
            f.restype, f.argtypes = res, args
        self.env = L.fj_env()
        self.natives = {}
        for d in java_natives():
            f = getattr(L, d["symbol"])
            f.restype = _CT.get(d["c_ret"], VP)
            f.argtypes = [VP, VP] + [_CT.get(t, VP) for t in d["c_params"][2:]]
            self.natives[d["name"]] = (f, d)
        self._keep = []   # memory under direct buffers
        self._dtype = {}  # array -> numpy dtype

    # -- objects
    def array(self, kind, values):
        code, dt = KINDS[kind]
        a = np.ascontiguousarray(values, dtype=dt) if not isinstance(values, np.ndarray) or values.dtype != dt else np.ascontiguousarray(values)
        h = self.L.fj_new_array(code, a.size, a.ctypes.data if a.size else None)
        self._dtype[h] = dt
        return h

    def object_array(self, handles):
        arr = (ctypes.c_void_p * max(1, len(handles)))(*handles)
        return self.L.fj_new_object_array(len(handles), arr)

    def buffer(self, a):
        """A direct ByteBuffer over a numpy array's memory."""
        a = np.ascontiguousarray(a)
        self._keep.append(a)
        return self.L.fj_new_direct_buffer(a.ctypes.data, a.nbytes)

    def heap_buffer(self):
        return self.L.fj_new_heap_buffer()

    def read_bytes(self, h):
        n = self.L.fj_array_bytes(h)
        return ctypes.string_at(self.L.fj_array_data(h), n) if n else b""

    def read(self, h, dtype=None):
        """The Java array's own contents (what the caller sees after the native returned), as a fresh numpy array."""
        return np.frombuffer(self.read_bytes(h), dtype=dtype or self._dtype[h]).copy()

    # -- calls
    def call(self, name, *args):
        """A native by its Java name; a String comes back as bytes, a byte[] as its object, null as None."""
        f, d = self.natives[name]
        assert len(args) == len(d["params"]), (name, len(args), len(d["params"]))
        self.L.fj_clear_exception()  # (Java code runs between two natives: nothing is pending when one is entered)
        r = f(self.env, None, *args)
        if d["c_ret"] == "jstring":
            return None if not r else self.L.fj_string_utf(r)
        return r

    # -- the outcome
    def pins(self):
        return self.L.fj_outstanding_pins()

    def faults(self):
        return self.L.fj_fault_log().decode()

    def assert_clean(self, what=""):
        assert self.pins() == 0, (what, "Get...Elements without a release: %d outstanding" % self.pins())
        assert self.L.fj_fault_count(-1) == 0, (what, self.faults())

    def reset(self):
        self.L.fj_reset()
        self._keep, self._dtype = [], {}


# ---- scripts ----------------------------------------------------------------------------------------------------------------------
# An op is a tuple; ids are small integers chosen by the script.
#   ("label", text)                       names what follows in a failure's message
#   ("array", id, kind, bytes)            a primitive array of len(bytes) / itemsize elements
#   ("objects", id, [id | None, ...])     an Object[] of earlier arrays
#   ("buffer", id, bytes)                 a direct buffer over memory holding those bytes
#   ("heap_buffer", id)                   a ByteBuffer that is not direct
#   ("gather", id, [id, ...])             a long[] holding the long at [0] of each of those arrays (handles made by earlier calls)
#   ("call", native, [arg, ...])          arg: ("o", id) object | None null | ("n", int) number | ("h", id) the long at [0] of array id
#   ("ret", int)                          the last call returned that int
#   ("ret_null",) ("ret_string", bytes) ("ret_bytes", bytes)   ... null / that String / a byte[] of those bytes
#   ("bytes", id, bytes)                  the Java array holds exactly those bytes now
#   ("nonzero", id) ("zero", id)          the long at [0] of array id
#   ("clean",)                            no outstanding pin, empty fault log
#   ("fail_gets", skip, count)            fj_fail_gets
#   ("fail_consumed",)                    every ordered NULL was handed out
#   ("gets_mark",) ("gets_exact", n, left)   run_ops() only: since the mark exactly n Get<T>ArrayElements calls, `left` ordered NULLs unused
ITEM = {"byte": 1, "char": 2, "short": 2, "int": 4, "long": 8, "float": 4}


def run_ops(fake, ops):
    objs, label, last, mark = {}, "", None, 0
    for op in ops:
        k = op[0]
        where = (label, op[:2])
        if k == "label":
            label = op[1]
        elif k == "array":
            objs[op[1]] = fake.array(op[2], np.frombuffer(op[3], dtype=KINDS[op[2]][1]))
        elif k == "objects":
            objs[op[1]] = fake.object_array([None if i is None else objs[i] for i in op[2]])
        elif k == "buffer":
            objs[op[1]] = fake.buffer(np.frombuffer(op[2], dtype=np.uint8).copy())
        elif k == "heap_buffer":
            objs[op[1]] = fake.heap_buffer()
        elif k == "gather":
            objs[op[1]] = fake.array("long", [int(fake.read(objs[i], np.int64)[0]) for i in op[2]])
        elif k == "call":
            args = []
            for a in op[2]:
                if a is None:
                    args.append(None)
                elif a[0] == "o":
                    args.append(objs[a[1]])
                elif a[0] == "n":
                    args.append(a[1])
                else:
                    args.append(int(fake.read(objs[a[1]], np.int64)[0]))
            last = fake.call(op[1], *args)
        elif k == "ret":
            assert last == op[1], (where, "returned", last, fake.call("lastError"))
        elif k == "ret_null":
            assert last is None, (where, "returned", last)
        elif k == "ret_string":
            assert last == op[1], (where, "returned", last)
        elif k == "ret_bytes":
            assert last is not None and fake.read_bytes(last) == op[1], (where, "the returned byte[] differs")
        elif k == "bytes":
            got = fake.read_bytes(objs[op[1]])
            assert got == op[2], (where, "array %d holds" % op[1], got[:64], "expected", op[2][:64])
        elif k in ("nonzero", "zero"):
            v = int(fake.read(objs[op[1]], np.int64)[0])
            assert (v != 0) == (k == "nonzero"), (where, v)
        elif k == "clean":
            fake.assert_clean(where)
        elif k == "fail_gets":
            fake.L.fj_fail_gets(op[1], op[2])
        elif k == "gets_mark":
            mark = fake.L.fj_get_calls()
        elif k == "gets_exact":
            made, left = fake.L.fj_get_calls() - mark, fake.L.fj_fail_gets_left()
            fake.L.fj_fail_gets(0, 0)
            assert made == op[1] and left == op[2], (where, "Get...Elements calls made", made, "the table says", op[1], "ordered NULLs left", left, "of", op[2])
        elif k == "fail_consumed":
            assert fake.L.fj_fail_gets_left() == 0, (where, "the native made fewer Get...Elements calls than the case expects")
            fake.L.fj_fail_gets(0, 0)
        else:
            raise ValueError(op)


def ops_text(ops):
    """The script as the sanitizer program reads it: one op per line, bytes as hex (`-`: none)."""
    hx = lambda b: b.hex() if b else "-"
    out = []
    for op in ops:
        k = op[0]
        if k == "label":
            out.append("label " + hx(op[1].encode()))
        elif k == "array":
            out.append("array %d %d %d %s" % (op[1], KINDS[op[2]][0], len(op[3]) // ITEM[op[2]], hx(op[3])))
        elif k == "objects":
            out.append("objects %d %d %s" % (op[1], len(op[2]), " ".join("-" if i is None else str(i) for i in op[2])))
        elif k == "buffer":
            out.append("buffer %d %d %s" % (op[1], len(op[2]), hx(op[2])))
        elif k == "heap_buffer":
            out.append("heap_buffer %d" % op[1])
        elif k == "gather":
            out.append("gather %d %d %s" % (op[1], len(op[2]), " ".join(str(i) for i in op[2])))
        elif k == "call":
            out.append("call %s %d %s" % (op[1], len(op[2]), " ".join("-" if a is None else {"o": "@", "n": "#", "h": "*"}[a[0]] + str(a[1]) for a in op[2])))
        elif k in ("ret_string", "ret_bytes"):
            out.append("%s %s" % (k, hx(op[1])))
        elif k == "bytes":
            out.append("bytes %d %s" % (op[1], hx(op[2])))
        else:
            out.append(" ".join(str(x) for x in op))
    return "\n".join(out) + "\n"


class Script:
    """Builds ops; remembers every array's initial bytes so that unchanged() can ask for them back."""

    def __init__(self):
        self.ops, self.next_id, self.initial = [], 1, {}

    def label(self, text):
        self.ops.append(("label", text))

    def array(self, kind, values):
        b = np.ascontiguousarray(values, dtype=KINDS[kind][1]).tobytes()
        i, self.next_id = self.next_id, self.next_id + 1
        self.ops.append(("array", i, kind, b))
        self.initial[i] = b
        return i

    def objects(self, ids):
        i, self.next_id = self.next_id, self.next_id + 1
        self.ops.append(("objects", i, list(ids)))
        return i

    def buffer(self, data):
        i, self.next_id = self.next_id, self.next_id + 1
        self.ops.append(("buffer", i, bytes(data)))
        return i

    def heap_buffer(self):
        i, self.next_id = self.next_id, self.next_id + 1
        self.ops.append(("heap_buffer", i))
        return i

    def gather(self, ids):
        i, self.next_id = self.next_id, self.next_id + 1
        self.ops.append(("gather", i, list(ids)))
        self.initial[i] = None  # (handles: known only when the script runs)
        return i

    def call(self, native, *args):
        self.ops.append(("call", native, list(args)))

    def add(self, *op):
        self.ops.append(tuple(op))

    def unchanged(self, ids):
        for i in ids:
            self.ops.append(("bytes", i, self.initial[i]))


def O(i):
    return None if i is None else ("o", i)


def N(v):
    return ("n", int(v))


def H(i):
    return ("h", i)


def u16(s):
    return np.frombuffer(s.encode("utf-16-le", "surrogatepass"), dtype=np.uint16)


# ---- the device-free natives against the ctypes path of needle_amd/_lib.py --------------------------------------------------------
GOOD_REGEXES = ["[0-9]+", "(ab|cd)+e?", "Sherlock|Holmes|Watson", "[\u8000-\u9000]+\uffff?", "\u4e2d\u6587|\u0416+"]
BAD_REGEXES = ["(", "[a-", "a{2,1}", "*a", "ab)", "\uffff(\u8000"]


def lib_compile(regex, flags=0):
    """-> (status, handle, last error) of needle_compile through ctypes."""
    from needle_amd import _lib
    L = _lib.lib()
    u = u16(regex)
    h = ctypes.c_void_p()
    rc = L.needle_compile(u.ctypes.data if u.size else None, u.size, flags, ctypes.byref(h))
    return rc, h.value, L.needle_last_error()


def lib_blob(handle):
    from needle_amd import _lib
    L = _lib.lib()
    need = ctypes.c_size_t()
    assert L.needle_pattern_serialize(handle, None, 0, ctypes.byref(need)) == 0
    buf = ctypes.create_string_buffer(need.value)
    assert L.needle_pattern_serialize(handle, buf, need.value, ctypes.byref(need)) == 0
    return buf.raw[:need.value]


def lib_tables(handle):
    """-> {cm: 65536 class-map bytes, stride, ns: n_states[4], mc: max_char[4], tables: 4 int16 arrays, accepting: 4 uint8 arrays, fixed_len}."""
    from needle_amd import _lib
    L = _lib.lib()
    info = _lib.PatternInfo()
    assert L.needle_pattern_get_info(handle, ctypes.byref(info)) == 0
    cm = np.zeros(65536, dtype=np.uint8)
    assert L.needle_pattern_get_class_map(handle, cm.ctypes.data) == 0
    tables, accepting = [], []
    for which in range(4):
        t = np.zeros(info.n_states[which] * info.stride, dtype=np.int16)
        a = np.zeros(info.n_states[which], dtype=np.uint8)
        assert L.needle_pattern_get_table(handle, which, t.ctypes.data, a.ctypes.data) == 0
        tables.append(t)
        accepting.append(a)
    return {"cm": cm, "stride": info.stride, "ns": np.array(list(info.n_states), dtype=np.int32), "mc": np.array(list(info.max_char), dtype=np.int32),
            "tables": tables, "accepting": accepting, "fixed_len": info.fixed_len}


def lib_from_tables(tb):
    from needle_amd import _lib
    L = _lib.lib()
    cm, stride, ns, mc, tables, accepting, fixed_len = (tb[k] for k in ("cm", "stride", "ns", "mc", "tables", "accepting", "fixed_len"))
    d = _lib.TableDesc()
    d.class_map, d.stride, d.fixed_len = cm.ctypes.data, stride, fixed_len
    for i, name in enumerate(("matches", "contained_in", "forwards", "backwards")):
        dd = getattr(d, name)
        dd.n_states, dd.max_char, dd.table, dd.accepting = int(ns[i]), int(mc[i]), tables[i].ctypes.data, accepting[i].ctypes.data
    h = ctypes.c_void_p()
    rc = L.needle_pattern_from_tables(ctypes.byref(d), ctypes.byref(h))
    return rc, h.value


def tables_args(s, tb, out):
    """The arguments of Native.fromTables for lib_tables()' result (an entry None: null; a list element None: a null element), as script
    objects -> (args, ids of every array)."""
    ids = []

    def arr(kind, v):
        if v is None:
            return None
        ids.append(s.array(kind, v))
        return ids[-1]

    def objs(kind, lst):
        return None if lst is None else s.objects([arr(kind, v) for v in lst])
    cm = tb["cm"]
    return ([O(arr("byte", None if cm is None else cm.view(np.int8))), N(tb["stride"]), O(arr("int", tb["ns"])), O(arr("int", tb["mc"])),
             O(objs("short", tb["tables"])), O(objs("byte", None if tb["accepting"] is None else [None if a is None else a.view(np.int8) for a in tb["accepting"]])),
             N(tb["fixed_len"]), O(out)], ids)


def device_free_ops():
    """compile / serialize / deserialize / fromTables / the info natives / setCreate through the shim, each expectation computed here through
    ctypes from the same library."""
    from needle_amd import _lib
    L = _lib.lib()
    s = Script()
    for regex in GOOD_REGEXES:
        rc, h, _ = lib_compile(regex)
        assert rc == 0, regex
        blob = lib_blob(h)
        s.label("compile %r" % regex)
        a_re, a_out = s.array("char", u16(regex)), s.array("long", [0x5A5A5A5A5A5A5A5A])
        s.call("compile", O(a_re), N(0), O(a_out))
        s.add("ret", 0), s.add("nonzero", a_out), s.add("clean"), s.unchanged([a_re])
        s.label("serialize %r" % regex)
        s.call("serialize", H(a_out))
        s.add("ret_bytes", blob), s.add("clean")
        s.label("deserialize %r" % regex)
        a_blob, a_out2 = s.array("byte", np.frombuffer(blob, dtype=np.int8)), s.array("long", [-1])
        s.call("deserialize", O(a_blob), O(a_out2))
        s.add("ret", 0), s.add("nonzero", a_out2), s.add("clean"), s.unchanged([a_blob])
        s.call("serialize", H(a_out2))
        s.add("ret_bytes", blob), s.add("clean")
        s.label("fromTables %r" % regex)
        tb = lib_tables(h)
        rc_ft, h_ft = lib_from_tables(tb)
        assert rc_ft == 0
        a_out3 = s.array("long", [-1])
        args, ids = tables_args(s, tb, a_out3)
        s.call("fromTables", *args)
        s.add("ret", 0), s.add("nonzero", a_out3), s.add("clean"), s.unchanged(ids)
        s.call("serialize", H(a_out3))
        s.add("ret_bytes", lib_blob(h_ft)), s.add("clean")
        # the info natives, field by field
        for which in (1, 2, 0, 5):
            pi = _lib.PrefilterInfo()
            rc_pi = L.needle_pattern_prefilter_info(h, which, ctypes.byref(pi), None)
            err = L.needle_last_error()
            s.label("prefilterInfo %r which %d" % (regex, which))
            a_info = s.array("int", [-7] * 7)
            s.call("prefilterInfo", H(a_out), N(which), O(a_info))
            if rc_pi == 0:
                s.add("ret_string", bytes(pi.why))
                s.add("bytes", a_info, np.array([pi.on, pi.mode, pi.stride, pi.warm, pi.min_len, pi.n_windows, pi.bitmap_bytes], dtype=np.int32).tobytes())
            else:
                s.add("ret_string", err), s.unchanged([a_info])
            s.add("clean")
            st = _lib.PrefilterState()
            rc_st = L.needle_pattern_prefilter_state(h, which, ctypes.byref(st))
            s.label("prefilterState %r which %d" % (regex, which))
            a_state, a_rate, a_counts = s.array("int", [-7] * 4), s.array("float", [-7.0]), s.array("long", [-7] * 2)
            s.call("prefilterState", H(a_out), N(which), O(a_state), O(a_rate), O(a_counts))
            s.add("ret", rc_st)
            if rc_st == 0:
                s.add("bytes", a_state, np.array([st.mode, st.has_filter, st.suspended_calls_left, st.backoff], dtype=np.int32).tobytes())
                s.add("bytes", a_rate, np.array([st.last_candidates_per_kib], dtype=np.float32).tobytes())
                s.add("bytes", a_counts, np.array([st.filter_launches, st.suspended_calls], dtype=np.int64).tobytes())
            else:
                s.unchanged([a_state, a_rate, a_counts])
            s.add("clean")
        for mode in (1, 2, 7, -1, 0):
            s.label("setPrefilter %r mode %d" % (regex, mode))
            s.call("setPrefilter", H(a_out), N(mode))
            s.add("ret", L.needle_pattern_set_prefilter(h, mode)), s.add("clean")
        page, sub = ctypes.c_int32(-9), ctypes.c_int32(-9)
        rc_r = L.needle_pattern_utf16_route(h, ctypes.byref(page), ctypes.byref(sub))
        s.label("utf16Route %r" % regex)
        a_route = s.array("int", [-9, -9])
        s.call("utf16Route", H(a_out), O(a_route))
        s.add("ret", rc_r), s.add("bytes", a_route, np.array([page.value, sub.value], dtype=np.int32).tobytes()), s.add("clean")
        for cw in (1, 2, 3):
            for count_only in (0, 1):
                av = ctypes.c_int32(-9)
                rc_f = L.needle_pattern_find_all_packed_filter(h, cw, count_only, ctypes.byref(av))
                s.label("findAllPackedFilter %r cw %d count_only %d" % (regex, cw, count_only))
                a_av = s.array("int", [-9])
                s.call("findAllPackedFilter", H(a_out), N(cw), N(count_only), O(a_av))
                s.add("ret", rc_f), s.add("bytes", a_av, np.array([av.value if rc_f == 0 else -9], dtype=np.int32).tobytes()), s.add("clean")
        for a in (a_out, a_out2, a_out3):
            s.call("destroyPattern", H(a))
        s.add("clean")
    for regex in BAD_REGEXES:
        rc, h, err = lib_compile(regex)
        assert rc != 0 and not h, regex
        s.label("compile (refused) %r" % regex)
        a_re, a_out = s.array("char", u16(regex)), s.array("long", [0x5A5A5A5A5A5A5A5A])
        s.call("compile", O(a_re), N(0), O(a_out))
        s.add("ret", rc), s.add("zero", a_out), s.add("clean"), s.unchanged([a_re])
        s.call("lastError")
        s.add("ret_string", err), s.add("clean")
    s.label("deserialize (refused)")
    junk = np.arange(100, dtype=np.int8)
    h_bad = ctypes.c_void_p()
    rc_bad = L.needle_pattern_deserialize(junk.ctypes.data, junk.size, ctypes.byref(h_bad))
    err_bad = L.needle_last_error()
    a_junk, a_out = s.array("byte", junk), s.array("long", [-1])
    s.call("deserialize", O(a_junk), O(a_out))
    s.add("ret", rc_bad), s.add("zero", a_out), s.add("clean")
    s.call("lastError")
    s.add("ret_string", err_bad)
    # tuningInfo, trimScratch
    need = ctypes.c_size_t()
    L.needle_tuning_info.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.POINTER(ctypes.c_size_t)]
    assert L.needle_tuning_info(None, 0, ctypes.byref(need)) == 0
    buf = ctypes.create_string_buffer(need.value)
    assert L.needle_tuning_info(buf, need.value, None) == 0
    s.label("tuningInfo")
    s.call("tuningInfo")
    s.add("ret_string", buf.value), s.add("clean")
    L.needle_trim_scratch.argtypes = [ctypes.c_size_t]
    for keep in (0, 1 << 20, -5):
        s.label("trimScratch %d" % keep)
        s.call("trimScratch", N(keep))
        s.add("ret", L.needle_trim_scratch(max(keep, 0))), s.add("clean")
    # setCreate / setDestroy: 0, 1, 3, 32 and 33 patterns
    handles = [lib_compile(r)[1] for r in ("a+", "[0-9]+", "x|yz")]
    a_h = [s.array("long", [-1]) for _ in handles]
    for r, a in zip(("a+", "[0-9]+", "x|yz"), a_h):
        s.call("compile", O(s.array("char", u16(r))), N(0), O(a))
        s.add("ret", 0)
    for k in (0, 1, 3, 32, 33):
        ps = (ctypes.c_void_p * max(k, 1))(*[handles[i % 3] for i in range(k)])
        out = ctypes.c_void_p()
        rc_s = L.needle_pattern_set_create(ps, k, ctypes.byref(out))
        s.label("setCreate of %d patterns" % k)
        a_set = s.array("long", [0])
        s.call("setCreate", O(s.gather([a_h[i % 3] for i in range(k)])), O(a_set))
        s.add("ret", rc_s), s.add("nonzero" if rc_s == 0 else "zero", a_set), s.add("clean")
        if rc_s == 0:
            s.call("setDestroy", H(a_set))
            s.add("clean")
            L.needle_pattern_set_destroy(out)
    for a in a_h:
        s.call("destroyPattern", H(a))
    s.add("clean")
    return s.ops


# ---- argument validation ----------------------------------------------------------------------------------------------------------
# One valid call per native that takes an array or a buffer, on 3 packed rows of 2, 0 and 3 chars (or 3 rows of stride 8).  An argument:
#   ("h",)                                   the handle of a compiled pattern
#   ("n", v)                                 a number
#   ("a", kind, values | length, required, need)   an array: required (null is refused) or optional; need: the least length the
#                                            header's contract asks for (None: any) -- one element fewer must be refused
#   ("offsets",)                             the packed batch's long[4]; required, and an empty one must be refused
#   ("b", nbytes, required)                  a direct buffer
N_ROWS, DATA, OFFSETS = 3, "ab123", [0, 2, 2, 5]
FIXED = [("h",), ("b", 24, True), ("n", 1), ("n", N_ROWS), ("n", 8), ("n", 8), ("b", 12, False)]
PACKED = [("a", "char", u16(DATA), True, 5), ("offsets",)]
PACKED8 = [("a", "byte", np.frombuffer(DATA.encode(), dtype=np.int8), True, 5), ("offsets",)]
BITMAP = ("a", "long", 1, True, 1)
# name -> (arguments, Get<T>ArrayElements calls of the valid call)
VALIDATION = {
    "compile": ([("a", "char", u16("ab"), True, None), ("n", 0), ("a", "long", 1, True, 1)], 1),
    "matchesHost": (FIXED + [BITMAP], 1),
    "containedInHost": (FIXED + [BITMAP], 1),
    "findHost": (FIXED + [BITMAP, ("a", "int", 3, True, 3), ("a", "int", 3, True, 3)], 3),
    "findAllHost": (FIXED + [("n", 2), ("a", "int", 3, True, 3), ("a", "int", 6, True, 6), ("a", "int", 6, True, 6), ("a", "int", 1, False, 1)], 3),
    "findAllPacked16Host": (FIXED + [("n", 2), ("a", "int", 3, True, 3), ("a", "int", 6, True, 6), ("a", "int", 1, False, 1)], 2),
    "findAllCsrHost": (FIXED + [("a", "long", 4, True, 4), ("a", "int", 4, False, None), ("a", "int", 4, False, None), ("a", "long", 1, True, 1)], 3),
    "findCompactHost": (FIXED + [BITMAP, ("a", "int", 6, False, None), ("a", "long", 1, True, 1)], 2),
    "findPacked16Host": (FIXED + [BITMAP, ("a", "int", 3, True, 3)], 2),
    "findPacked8Host": (FIXED + [BITMAP, ("a", "short", 3, True, 3)], 2),
    "packedHost": ([("h",), ("n", 2)] + PACKED + [BITMAP, ("a", "int", 3, True, 3), ("a", "int", 3, True, 3)], 5),
    "findAllPackedHost": ([("h",)] + PACKED + [("a", "long", 4, True, 4), ("a", "int", 4, False, None), ("a", "int", 4, False, None), ("a", "long", 1, True, 1)], 5),
    "findAllUtf8PackedHost": ([("h",)] + PACKED8 + [("a", "long", 4, True, 4), ("a", "int", 4, False, None), ("a", "int", 4, False, None), ("a", "long", 1, True, 1),
                                                  ("a", "long", 1, False, 1)], 6),
    "containedInUtf8PackedHost": ([("h",)] + PACKED8 + [BITMAP, ("a", "long", 1, False, 1)], 4),
    "replaceAllPackedHost": ([("h",)] + PACKED + [("a", "char", u16("xy"), True, None), ("a", "long", 4, True, 4), ("a", "char", 8, False, None), ("a", "long", 1, True, 1)], 5),
    "gatherMatchesPackedHost": ([("h",)] + PACKED + [("n", 0), ("a", "long", 4, True, 4), ("a", "long", 5, False, None), ("a", "char", 8, False, None),
                                                   ("a", "long", 2, True, 2)], 5),
    "findPacked16PackedHost": ([("h",)] + PACKED + [BITMAP, ("a", "int", 3, True, 3)], 4),
    "findPacked8PackedHost": ([("h",)] + PACKED + [BITMAP, ("a", "short", 3, True, 3)], 4),
    "setCreate": ([("a", "long", "handle", True, 1), ("a", "long", 1, True, 1)], 1),
    "setPackedHost": ([("n", 0), ("n", 0)] + PACKED + [("a", "int", 3, True, 3)], 3),
    "setTagMatchesPackedHost": ([("n", 0), ("h",)] + PACKED + [("a", "long", 4, True, 4), ("a", "int", 4, False, None), ("a", "int", 4, False, None),
                                                             ("a", "int", 4, False, None), ("a", "long", 1, True, 1)], 6),
    "setReplaceEachPackedHost": ([("n", 0), ("h",)] + PACKED + [("a", "char", u16("xy"), True, None), ("a", "int", [0, 1, 2], True, 2), ("a", "long", 4, True, 4),
                                                              ("a", "char", 8, False, None), ("a", "long", 1, True, 1)], 6),
    "deserialize": ([("a", "byte", "blob", True, None), ("a", "long", 1, True, 1)], 1),
    "multiCreate": ([("a", "int", [0], True, None), ("n", 0), ("a", "long", 1, True, 1)], 1),
    "scanHostMulti": ([("n", 0), ("h",), ("n", 2)] + FIXED[1:] + [BITMAP, ("a", "int", 3, True, 3), ("a", "int", 3, True, 3)], 3),
    "matcherCreate": ([("h",), ("a", "char", u16("ab"), True, None), ("a", "long", 1, True, 1)], 1),
    "matcherMatches": ([("n", 0), ("a", "int", 1, True, 1)], 0),
    "matcherContainedIn": ([("n", 0), ("a", "int", 1, True, 1)], 0),
    "matcherFind": ([("n", 0), ("a", "int", 1, True, 1)], 0),
    "matcherFindRange": ([("n", 0), ("n", 0), ("n", 1), ("a", "int", 1, True, 1)], 0),
    "prefilterState": ([("h",), ("n", 1), ("a", "int", 4, False, 4), ("a", "float", 1, False, 1), ("a", "long", 2, False, 2)], 0),
    "findAllPackedFilter": ([("h",), ("n", 1), ("n", 0), ("a", "int", 1, True, 1)], 0),
    "utf16Route": ([("h",), ("a", "int", 2, True, 2)], 0),
}
# natives whose arrays the generic table cannot describe, or that return no status; validation_ops() writes their cases by hand
VALIDATION_BY_HAND = ("fromTables", "prefilterInfo", "serialize")


def garbage(kind, n, salt):
    b = bytes((i * 37 + 11 + salt) & 0xFF for i in range(n * ITEM[kind]))
    return np.frombuffer(b, dtype=KINDS[kind][1])


# the native that frees what a valid call of these natives makes, and the argument that holds the handle
DESTROYERS = {"compile": ("destroyPattern", 2), "deserialize": ("destroyPattern", 1), "setCreate": ("setDestroy", 1), "multiCreate": ("multiDestroy", 2),
              "matcherCreate": ("matcherDestroy", 2)}


def validation_ops(get_counts=False):
    """get_counts: instead of the cases below, ONE valid call per native with Get<T>ArrayElements ordered to return NULL from call
    number `gets` + 1 on: the native must make exactly `gets` calls and none of the ordered NULLs may be handed out -- so the table's
    counts, which decide how many positions the cases below try, are the shim's own.  (These calls go on into the library; without
    a device its scan entries answer NEEDLE_ERR_DEVICE.  run_ops() only, not for the sanitizer program.)
    For every native of VALIDATION: each required argument null, each array one element short of its contract, empty offsets, a heap
    buffer for each direct one, and Get<T>ArrayElements returning NULL at every position -- all NEEDLE_ERR_INVALID, nothing pinned, no
    fault, every array as it was.  None of these reaches the library's scan entries."""
    s = Script()
    a_h = s.array("long", [0])
    s.call("compile", O(s.array("char", u16("[0-9]+"))), N(0), O(a_h))
    s.add("ret", 0)
    rc, h, _ = lib_compile("[0-9]+")
    blob = np.frombuffer(lib_blob(h), dtype=np.int8)

    def case(name, spec, what, null=None, short=None, empty_offsets=False, heap=None, fail_at=None, expect=("ret", ERR_INVALID)):
        s.label("%s: %s" % (name, what))
        args, arrays = [], []
        for i, a in enumerate(spec):
            if a[0] == "h":
                args.append(H(a_h))
            elif a[0] == "n":
                args.append(N(a[1]))
            elif i == null:
                args.append(None)
            elif a[0] == "b":
                args.append(O(s.heap_buffer() if i == heap else s.buffer(bytes(garbage("byte", a[1], i).tobytes()))))
            elif a[0] == "offsets":
                arrays.append(s.array("long", [] if empty_offsets else OFFSETS))
                args.append(O(arrays[-1]))
            else:
                _, kind, values, _, need = a
                if isinstance(values, str) and values == "handle":  # (a long[] of pattern handles: the script's own)
                    arrays.append(s.gather([] if i == short else [a_h]))
                else:
                    values = np.asarray(blob if isinstance(values, str) else garbage(kind, values, i) if isinstance(values, int) else values)
                    arrays.append(s.array(kind, values[:need - 1] if i == short else values))
                args.append(O(arrays[-1]))
        if get_counts:
            s.add("gets_mark"), s.add("fail_gets", VALIDATION[name][1], 1000)
            s.call(name, *args)
            s.add("gets_exact", VALIDATION[name][1], 1000), s.add("clean")
            if name in DESTROYERS:
                s.call(DESTROYERS[name][0], ("h", args[DESTROYERS[name][1]][1]))
            return
        if fail_at is not None:
            s.add("fail_gets", fail_at, 1)
        s.call(name, *args)
        s.add(*expect)
        if fail_at is not None:
            s.add("fail_consumed")
        s.add("clean")
        s.unchanged([i for i in arrays if s.initial[i] is not None])

    if get_counts:
        for name, (spec, gets) in VALIDATION.items():
            case(name, spec, "the Get...Elements calls of a valid call")
        s.label("serialize: the Get...Elements calls of a valid call")
        s.add("gets_mark"), s.add("fail_gets", 1, 1000)
        s.call("serialize", H(a_h))
        s.add("gets_exact", 1, 1000), s.add("clean")
        s.label("fromTables: the Get...Elements calls of a valid call")
        out = s.array("long", [-1])
        args, _ = tables_args(s, lib_tables(h), out)
        s.add("gets_mark"), s.add("fail_gets", 9, 1000)
        s.call("fromTables", *args)
        s.add("gets_exact", 9, 1000), s.add("ret", 0), s.add("clean")
        s.call("destroyPattern", H(out))
        s.call("destroyPattern", H(a_h))
        return s.ops

    for name, (spec, gets) in VALIDATION.items():
        for i, a in enumerate(spec):
            if a[0] == "offsets" or (a[0] in ("a", "b") and a[-2 if a[0] == "a" else -1]):
                case(name, spec, "argument %d null" % i, null=i)
            if a[0] == "a" and a[4]:
                case(name, spec, "argument %d one element short (%d)" % (i, a[4] - 1), short=i)
            if a[0] == "offsets":
                case(name, spec, "empty offsets", empty_offsets=True)
            if a[0] == "b":
                case(name, spec, "argument %d a heap buffer" % i, heap=i)
        for k in range(gets):
            case(name, spec, "Get...Elements call %d of %d returns NULL" % (k + 1, gets), fail_at=k)
    # prefilterInfo returns a String: a short info gives null; serialize returns a byte[]: null when its one Get fails
    case("prefilterInfo", [("h",), ("n", 1), ("a", "int", 7, False, 7)], "info one element short", short=2, expect=("ret_null",))
    s.label("serialize: Get...Elements returns NULL")
    s.add("fail_gets", 0, 1)
    s.call("serialize", H(a_h))
    s.add("ret_null"), s.add("fail_consumed"), s.add("clean")
    # fromTables: nine arrays, eight of them inside Object[]s
    tb = lib_tables(h)

    def from_tables(what, fail_at=None, out_len=1, **changed):
        s.label("fromTables: " + what)
        out = s.array("long", [-1] * out_len)
        args, ids = tables_args(s, dict(tb, **changed), out)
        if fail_at is not None:
            s.add("fail_gets", fail_at, 1)
        s.call("fromTables", *args)
        s.add("ret", ERR_INVALID)
        if fail_at is not None:
            s.add("fail_consumed")
        s.add("clean")
        s.unchanged(ids + [out])

    def without(lst, i, v=None):
        return [v if j == i else x for j, x in enumerate(lst)]
    for key in ("cm", "ns", "mc", "tables", "accepting"):
        from_tables(key + " null", **{key: None})
    s.label("fromTables: handleOut null")
    args, ids = tables_args(s, tb, None)
    s.call("fromTables", *args)
    s.add("ret", ERR_INVALID), s.add("clean"), s.unchanged(ids)
    from_tables("handleOut empty", out_len=0)
    from_tables("a class map of 65535 bytes", cm=tb["cm"][:65535])
    from_tables("nStates of 3", ns=tb["ns"][:3])
    from_tables("maxChar of 3", mc=tb["mc"][:3])
    from_tables("tables of 3", tables=tb["tables"][:3])
    from_tables("accepting of 3", accepting=tb["accepting"][:3])
    from_tables("tables[2] null", tables=without(tb["tables"], 2))
    from_tables("accepting[1] null", accepting=without(tb["accepting"], 1))
    from_tables("tables[1] one element short", tables=without(tb["tables"], 1, tb["tables"][1][:-1]))
    from_tables("accepting[3] one element short", accepting=without(tb["accepting"], 3, tb["accepting"][3][:-1]))
    from_tables("stride 0", stride=0)
    from_tables("nStates[0] larger than its table", ns=np.array([tb["ns"][0] + 1] + list(tb["ns"][1:]), dtype=np.int32))
    for k in range(9):
        from_tables("Get...Elements call %d of 9 returns NULL" % (k + 1), fail_at=k)
    s.call("destroyPattern", H(a_h))
    s.add("clean")
    return s.ops


def dispatch_source():
    """jni_shim_dispatch.inc of tests/c/jni_shim_check.c: a prototype per native, as Native.java declares it, and dispatch()."""
    out, body = [], []
    for d in java_natives():
        out.append("%s %s(%s);" % (d["c_ret"], d["symbol"], ", ".join(d["c_params"])))
        args = ["env", "NULL"] + ["a[%d].o" % i if t.endswith("Array") or t in ("jobject", "jstring") else "(%s)a[%d].n" % (t, i)
                                  for i, t in enumerate(d["c_params"][2:])]
        macro = {"void": "R_VOID", "jint": "R_INT", "jlong": "R_INT"}.get(d["c_ret"], "R_OBJ")
        body.append('    if (!strcmp(name, "%s") && argc == %d) { %s(%s(%s)); return 1; }' % (d["name"], len(d["params"]), macro, d["symbol"], ", ".join(args)))
    return "\n".join(out + ["static int dispatch(JNIEnv *env, const char *name, int argc, const arg *a) {"] + body + ["    (void)env; (void)a; (void)argc;", "    return 0;", "}"]) + "\n"
