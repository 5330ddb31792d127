"""Host-side mirror of the reference's interface for this path, over the C ABI (include/needle_hip.h):

    DFACompiler.compile(regex, className[, flags]) -> Pattern   needle-compiler/.../DFACompiler.java:16-37
    Pattern.matcher(String) -> Matcher, flag constants          needle-types/.../Pattern.java:3-34
    Matcher.matches/containedIn/find/find(int,int)/start/end    needle-types/.../Matcher.java:6-26

plus the batch entry points the reference does not have (one launch over many haystacks).  Everything that
matches goes through the HIP kernels; nothing here walks an automaton on the CPU.
"""
import ctypes

import numpy as np

from . import _lib
from ._lib import BatchView, DfaDesc, PatternInfo, TableDesc

# flag constants, same values as the reference (Pattern.java:9-31)
CASE_INSENSITIVE = 0x02
DOTALL = 0x20
UNICODE_CASE = 0x40
UNICODE_CHARACTER_CLASS = 0x100
LEFTMOST_LONGEST = 0x800000
ALL_FLAGS = DOTALL | CASE_INSENSITIVE | UNICODE_CASE | LEFTMOST_LONGEST | UNICODE_CHARACTER_CLASS
# find() of packed rows in one dword / one uint16 (needle_find_packed{16,8}_packed_*): a match the form cannot hold
PACK16_OVER = 0xFFFEFFFF
PACK8_OVER = 0xFFFD


class PatternException(RuntimeError):
    """NC/PatternException.java"""


class PatternSyntaxException(PatternException):
    """NC/PatternSyntaxException.java (RegexParser.java:86-98,293-295)"""


class PatternClassCompilationException(PatternException):
    """NC/PatternClassCompilationException.java (DFACompiler.java:34-36,71-83)"""


class DeviceError(RuntimeError):
    """HIP failure / no device (IllegalStateException in the Java shim)."""


def _check(rc):
    if rc == _lib.NEEDLE_OK:
        return
    msg = _lib.last_error()
    if rc == _lib.ERR_INVALID:
        raise ValueError(msg)
    if rc == _lib.ERR_SYNTAX:
        raise PatternSyntaxException(msg)
    if rc in (_lib.ERR_COMPILE, _lib.ERR_UNSUPPORTED):
        raise PatternClassCompilationException(msg)
    raise DeviceError(msg)


def _utf16(s):
    """str -> uint16 code units (surrogate pairs for astral chars, like java.lang.String)."""
    if isinstance(s, np.ndarray):
        return np.ascontiguousarray(s, dtype=np.uint16)
    return np.frombuffer(s.encode("utf-16-le", "surrogatepass"), dtype=np.uint16).copy()


class Matcher:
    """One haystack + cursor (the generated class's fields, DFAClassBuilder.java:688-699)."""

    def __init__(self, pattern, s):
        self._pattern = pattern  # keeps the native pattern alive
        self._units = _utf16(s)
        h = ctypes.c_void_p()
        _check(_lib.lib().needle_matcher_create(pattern._h, self._units.ctypes.data, self._units.size, ctypes.byref(h)))
        self._h = h

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h and _lib is not None and _lib._lib is not None:  # module globals may be gone at interpreter exit
            _lib._lib.needle_matcher_destroy(h)

    def _bool(self, fn, *args):
        r = ctypes.c_int(0)
        _check(fn(self._h, *args, ctypes.byref(r)))
        return bool(r.value)

    def matches(self):
        return self._bool(_lib.lib().needle_matcher_matches)

    def containedIn(self):
        return self._bool(_lib.lib().needle_matcher_contained_in)

    def find(self, start=None, end=None):
        if start is None:
            return self._bool(_lib.lib().needle_matcher_find)
        return self._bool(_lib.lib().needle_matcher_find_range, int(start), int(end))

    def start(self):
        return _lib.lib().needle_matcher_start(self._h)

    def end(self):
        return _lib.lib().needle_matcher_end(self._h)


WHICH = {"matches": 0, "contained_in": 1, "forwards": 2, "backwards": 3}


class Pattern:
    """A compiled pattern: immutable, shareable, tables resident in HBM per device."""

    def __init__(self, handle, regex=None, flags=0):
        self._h = handle
        self.regex = regex
        self.flags = flags

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h and _lib is not None and _lib._lib is not None:
            _lib._lib.needle_pattern_destroy(h)

    # ---- reference interface
    def matcher(self, s):
        return Matcher(self, s)

    # ---- construction from the tables a generated class carries
    @classmethod
    def from_tables(cls, class_map, stride, dfas, fixed_len=-1):
        """dfas: {"matches"|"contained_in"|"forwards"|"backwards": dict(n_states, max_char, accepting (ids),
        table (flat int16) | table_strings (list[str]))}"""
        cm = np.ascontiguousarray(class_map, dtype=np.uint8)
        assert cm.size == 65536
        keep = [cm]
        desc = TableDesc()
        desc.class_map = cm.ctypes.data
        desc.stride = int(stride)
        desc.fixed_len = -1 if fixed_len is None else int(fixed_len)
        for name in WHICH:
            spec = dfas[name]
            d = DfaDesc()
            d.n_states = int(spec["n_states"])
            d.max_char = 0xFFFF if spec.get("max_char") is None else int(spec["max_char"])
            acc = np.zeros(d.n_states, dtype=np.uint8)
            for s in spec["accepting"]:
                acc[int(s)] = 1
            keep.append(acc)
            d.accepting = acc.ctypes.data
            if spec.get("table") is not None:
                t = np.ascontiguousarray(spec["table"], dtype=np.int16)
                assert t.size == d.n_states * desc.stride
                keep.append(t)
                d.table = t.ctypes.data
                d.table_string = None
            else:
                d.table = None
                d.table_string = ";".join(spec["table_strings"]).encode("ascii")
            setattr(desc, name, d)
        h = ctypes.c_void_p()
        _check(_lib.lib().needle_pattern_from_tables(ctypes.byref(desc), ctypes.byref(h)))
        del keep
        return cls(h)

    # ---- precompiled-pattern blob (the analogue of Precompile.precompile, NC/precompile/Precompile.java:19-53)
    def to_bytes(self):
        need = ctypes.c_size_t(0)
        _check(_lib.lib().needle_pattern_serialize(self._h, None, 0, ctypes.byref(need)))
        buf = (ctypes.c_ubyte * need.value)()
        _check(_lib.lib().needle_pattern_serialize(self._h, buf, need.value, ctypes.byref(need)))
        return bytes(buf)

    @classmethod
    def from_bytes(cls, blob):
        h = ctypes.c_void_p()
        b = (ctypes.c_ubyte * len(blob)).from_buffer_copy(blob)
        _check(_lib.lib().needle_pattern_deserialize(b, len(blob), ctypes.byref(h)))
        return cls(h)

    # ---- introspection
    def info(self):
        i = PatternInfo()
        _check(_lib.lib().needle_pattern_get_info(self._h, ctypes.byref(i)))
        return {"stride": i.stride, "n_states": dict(zip(WHICH, i.n_states)), "max_char": dict(zip(WHICH, i.max_char)),
                "fixed_len": i.fixed_len, "min_len": i.min_len, "max_len": i.max_len,
                "kernel_mode": dict(zip(WHICH, i.kernel_mode))}

    def program_info(self, which="forwards", char_width=1, with_backward=True):
        """How one automaton is lowered for the device (host-side diagnostics: needs no GPU)."""
        i = _lib.ProgramInfo()
        _check(_lib.lib().needle_pattern_program_info(self._h, list(WHICH).index(which), char_width, int(with_backward), ctypes.byref(i)))
        return {k: getattr(i, k) for k, _ in i._fields_}

    def prefilter_info(self, which="forwards", with_bitmap=False, wide=False):
        """The n-gram candidate filter behind which containedIn() / find() run on batches of 8-bit rows (SURVEY.md s8 f-4;
        host-side diagnostics: needs no GPU): {"on", "mode", "stride", "warm", "min_len", "n_windows", "bitmap_bytes", hash
        parameters, "why" (what ruled it out)} and, with_bitmap, "bitmap" (uint32 words).  wide: the filter of UTF-16 rows of a
        pattern on several pages of the BMP (windows of four code units: "m1b", "m2b" -- needle_pattern_prefilter_info2)."""
        i2 = _lib.PrefilterInfo2()
        L = _lib.lib()
        wi = list(WHICH).index(which)
        _check(L.needle_pattern_prefilter_info2(self._h, wi, int(bool(wide)), ctypes.byref(i2), None, 0))
        i = i2.base
        out = {k: getattr(i, k) for k, _ in i._fields_}
        out["why"] = out["why"].decode()
        out["wide"], out["m1b"], out["m2b"] = int(i2.wide), int(i2.m1b), int(i2.m2b)
        if with_bitmap and i.on:
            bm = np.zeros((i.bitmap_bytes + (i.bitmap2_bytes if i.on2 else 0)) // 4, dtype=np.uint32)
            _check(L.needle_pattern_prefilter_info2(self._h, wi, int(bool(wide)), ctypes.byref(i2), bm.ctypes.data, bm.size))
            out["bitmap"] = bm[:i.bitmap_bytes // 4]
            if i.on2:
                out["bitmap2"] = bm[i.bitmap_bytes // 4:]  # the second level's (5-byte windows)
        return out

    PREFILTER_AUTO, PREFILTER_ON, PREFILTER_OFF = 0, 1, 2

    def set_prefilter(self, mode):
        """needle_pattern_set_prefilter: AUTO (the flood watch decides), ON (the filter kernel whenever the shape allows, never suspended),
        OFF (the ordinary scan kernels).  Answers are the same in all three."""
        _check(_lib.lib().needle_pattern_set_prefilter(self._h, int(mode)))

    def prefilter_state(self, which="forwards"):
        """needle_pattern_prefilter_state: what the flood watch of this pattern's filter program knows on the current device."""
        st = _lib.PrefilterState()
        _check(_lib.lib().needle_pattern_prefilter_state(self._h, list(WHICH).index(which), ctypes.byref(st)))
        return {k: getattr(st, k) for k, _ in st._fields_}

    def utf16_route(self):
        """needle_pattern_utf16_route: (page, sub) -- UTF-16 rows of this pattern can run behind the byte program of BMP page `page` (0: ASCII /
        Latin-1, 4: Cyrillic ...), every char outside the page narrowed to byte `sub`; None when the pattern spans several pages.  No GPU needed."""
        page, sub = ctypes.c_int32(0), ctypes.c_int32(0)
        _check(_lib.lib().needle_pattern_utf16_route(self._h, ctypes.byref(page), ctypes.byref(sub)))
        return None if page.value < 0 else (page.value, sub.value)

    def match_length_automaton(self):
        """The refined forward automaton behind find-all's "lengths" form (needle_pattern_match_lengths), or None when the
        pattern does not allow it -> {"n_states", "n_dead", "max_char", "table" int16[n, stride + 1] (last column: chars beyond max_char), "accepting"
        bool[n], "pend" uint8[n]}."""
        L = _lib.lib()
        avail, n, nd, mc = ctypes.c_int32(0), ctypes.c_int32(0), ctypes.c_int32(0), ctypes.c_int32(0)
        _check(L.needle_pattern_match_lengths(self._h, ctypes.byref(avail), ctypes.byref(n), ctypes.byref(nd), ctypes.byref(mc), None, None, None))
        if not avail.value:
            return None
        stride = self.info()["stride"]
        table = np.zeros(n.value * (stride + 1), dtype=np.int16)
        acc = np.zeros(n.value, dtype=np.uint8)
        pend = np.zeros(n.value, dtype=np.uint8)
        _check(L.needle_pattern_match_lengths(self._h, ctypes.byref(avail), ctypes.byref(n), ctypes.byref(nd), ctypes.byref(mc), table.ctypes.data,
                                              acc.ctypes.data, pend.ctypes.data))
        return {"n_states": n.value, "n_dead": nd.value, "max_char": mc.value, "table": table.reshape(n.value, stride + 1),
                "accepting": acc.astype(bool), "pend": pend}

    def find_all_transducer(self, char_width=1):
        """The device program of the find-all transducer (needle_pattern_find_all_transducer: lock-step find-all), or None when the
        pattern has none -> {"n_states", "n_cols", "pad_col", "start", "window", "win_lo_e", "win_hi_e", "off_table", "codes_off",
        "lds_bytes", "n_pages", "kind" (1: the transducer on the lengths automaton -- a code names (length, k); 2: the RUN transducer of
        patterns without bounded match lengths -- code bit 0: a match ends in front of this char, bit 1: this char may begin a run),
        "blob": uint8[lds_bytes]}."""
        L = _lib.lib()
        avail, need = ctypes.c_int32(0), ctypes.c_size_t(0)
        info = (ctypes.c_int32 * 12)()
        _check(L.needle_pattern_find_all_transducer(self._h, int(char_width), ctypes.byref(avail), info, None, 0, ctypes.byref(need)))
        if not avail.value:
            return None
        blob = np.zeros(need.value, dtype=np.uint8)
        _check(L.needle_pattern_find_all_transducer(self._h, int(char_width), ctypes.byref(avail), info, blob.ctypes.data, blob.size, ctypes.byref(need)))
        keys = ["n_states", "n_cols", "pad_col", "start", "window", "win_lo_e", "win_hi_e", "off_table", "codes_off", "lds_bytes", "n_pages", "kind"]
        out = {k: int(info[i]) for i, k in enumerate(keys)}
        out["blob"] = blob
        return out

    def find_all_packed_route(self, char_width=1, count_only=False):
        """The route count_matches_packed (count_only) / find_all_packed take for this pattern on packed device rows of char_width
        (needle_pattern_find_all_packed_route; no device needed): "conversion" (to fixed-stride rows, offsets read back), "transducer"
        (the lock-step transducer kernel) or "lane" (the per-lane restart kernel)."""
        route = ctypes.c_int32(0)
        _check(_lib.lib().needle_pattern_find_all_packed_route(self._h, int(char_width), 1 if count_only else 0, ctypes.byref(route)))
        return ("conversion", "transducer", "lane")[route.value]

    def find_all_packed_filter(self, char_width=1, count_only=False):
        """Whether count_matches_packed (count_only) / find_all_packed take the n-gram filter kernel's find-all form for this pattern on
        packed device rows of char_width (needle_pattern_find_all_packed_filter; no device needed): neither the transducer nor the
        per-lane kernel takes it and the filter has a program for it.  The flood watch and set_prefilter are runtime state, left aside."""
        available = ctypes.c_int32(0)
        _check(_lib.lib().needle_pattern_find_all_packed_filter(self._h, int(char_width), 1 if count_only else 0, ctypes.byref(available)))
        return bool(available.value)

    def tables(self):
        """The pattern's tables in the reference layout (class map, stride, 4 x (table, accepting, max_char))."""
        inf = self.info()
        cm = np.zeros(65536, dtype=np.uint8)
        _check(_lib.lib().needle_pattern_get_class_map(self._h, cm.ctypes.data))
        out = {"class_map": cm, "stride": inf["stride"], "fixed_len": inf["fixed_len"], "min_len": inf["min_len"],
               "max_len": inf["max_len"], "dfas": {}}
        for name, w in WHICH.items():
            n = inf["n_states"][name]
            t = np.zeros(n * inf["stride"], dtype=np.int16)
            a = np.zeros(n, dtype=np.uint8)
            _check(_lib.lib().needle_pattern_get_table(self._h, w, t.ctypes.data, a.ctypes.data))
            out["dfas"][name] = {"n_states": n, "table": t, "accepting": np.nonzero(a)[0].tolist(),
                                 "max_char": inf["max_char"][name]}
        return out

    # ---- batches
    def _run(self, op, rows, lengths, stream, out=None):
        L = _lib.lib()
        v = BatchView()
        if isinstance(rows, np.ndarray):  # host buffers: upload + run + download inside the library
            rows = np.ascontiguousarray(rows)
            if rows.dtype == np.int16:
                rows = rows.view(np.uint16)
            assert rows.ndim == 2 and rows.dtype in (np.uint8, np.uint16), "rows: 2-D uint8/uint16"
            n, stride = rows.shape
            v.rows, v.char_width, v.n_rows, v.row_stride, v.row_len = rows.ctypes.data, rows.dtype.itemsize, n, stride, stride
            if lengths is not None:
                lengths = np.ascontiguousarray(lengths, dtype=np.uint32)
                assert lengths.shape == (n,)
                v.lengths = lengths.ctypes.data
            words = np.zeros((n + 63) // 64, dtype=np.uint64)
            if op == "find":
                st = np.full(n, -1, dtype=np.int32)
                en = np.full(n, -1, dtype=np.int32)
                _check(L.needle_find_host(self._h, ctypes.byref(v), words.ctypes.data, st.ctypes.data, en.ctypes.data))
                return words, st, en
            fn = L.needle_matches_host if op == "matches" else L.needle_contained_in_host
            _check(fn(self._h, ctypes.byref(v), words.ctypes.data))
            return words
        import torch  # device tensors: plumbing only (memory + stream)
        assert isinstance(rows, torch.Tensor) and rows.is_cuda and rows.dim() == 2 and rows.is_contiguous()
        assert rows.dtype in (torch.uint8, torch.int16, torch.uint16), "rows: uint8 or (u)int16 code units"
        n, stride = rows.shape
        cw = rows.element_size()
        v.rows, v.char_width, v.n_rows, v.row_stride, v.row_len = rows.data_ptr(), cw, n, stride, stride
        if lengths is not None:
            assert lengths.is_cuda and lengths.dtype == torch.int32 and lengths.shape == (n,) and lengths.is_contiguous()
            v.lengths = lengths.data_ptr()
        with torch.cuda.device(rows.device):
            s = torch.cuda.current_stream(rows.device).cuda_stream if stream is None else stream
            if out is not None:  # caller-owned result buffers (at least as large as the results): no allocation per call
                words = out[0] if isinstance(out, (tuple, list)) else out
                assert words.is_cuda and words.dtype == torch.int64 and words.numel() >= (n + 63) // 64
            else:
                words = torch.empty((n + 63) // 64, dtype=torch.int64, device=rows.device)
            if op == "find":
                if out is not None:
                    st, en = out[1], out[2]
                    assert st.dtype == torch.int32 and en.dtype == torch.int32 and st.numel() >= n and en.numel() >= n
                else:
                    st = torch.empty(n, dtype=torch.int32, device=rows.device)
                    en = torch.empty(n, dtype=torch.int32, device=rows.device)
                _check(L.needle_find_dev(self._h, ctypes.byref(v), words.data_ptr(), st.data_ptr(), en.data_ptr(), s))
                return words, st, en
            fn = L.needle_matches_dev if op == "matches" else L.needle_contained_in_dev
            _check(fn(self._h, ctypes.byref(v), words.data_ptr(), s))
            return words

    def matches_batch(self, rows, lengths=None, stream=None, out=None):
        """bitmap words (bit r&63 of word r>>6 = matches() of row r).  out: optional caller-owned int64 device tensor
        for the bitmap words (device batches only)."""
        return self._run("matches", rows, lengths, stream, out)

    def contained_in_batch(self, rows, lengths=None, stream=None, out=None):
        return self._run("contained_in", rows, lengths, stream, out)

    def find_next_batch(self, rows, cursor, lengths=None, stream=None):
        """One Matcher.find() step per row from the per-row cursor (int32 device tensor; < 0 = exhausted).
        -> (bitmap words, start, end); `end` is the rows' next cursor (-1 where nothing was found)."""
        import torch
        L = _lib.lib()
        assert isinstance(rows, torch.Tensor) and rows.is_cuda and rows.dim() == 2 and rows.is_contiguous()
        assert cursor.is_cuda and cursor.dtype == torch.int32 and cursor.shape == (rows.shape[0],) and cursor.is_contiguous()
        v = BatchView()
        n, stride = rows.shape
        v.rows, v.char_width, v.n_rows, v.row_stride, v.row_len = rows.data_ptr(), rows.element_size(), n, stride, stride
        if lengths is not None:
            assert lengths.is_cuda and lengths.dtype == torch.int32 and lengths.shape == (n,)
            v.lengths = lengths.data_ptr()
        with torch.cuda.device(rows.device):
            s = torch.cuda.current_stream(rows.device).cuda_stream if stream is None else stream
            words = torch.empty((n + 63) // 64, dtype=torch.int64, device=rows.device)
            st = torch.empty(n, dtype=torch.int32, device=rows.device)
            en = torch.empty(n, dtype=torch.int32, device=rows.device)
            _check(L.needle_find_next_dev(self._h, ctypes.byref(v), cursor.data_ptr(), words.data_ptr(), st.data_ptr(),
                                          en.data_ptr(), s))
        return words, st, en

    def find_all_dense(self, rows, max_per_row, lengths=None, stream=None, out=None):
        """needle_find_all_dev: every non-overlapping match of every row in dense per-row slots.
        -> (counts int32[n], start int32[n, max_per_row], end int32[n, max_per_row], more: bool)
        out: optional caller-owned (counts, start, end) device tensors (slots beyond a row's count are left as they are)."""
        L = _lib.lib()
        if isinstance(rows, np.ndarray):  # host buffers: needle_find_all_host
            rows = np.ascontiguousarray(rows)
            if rows.dtype == np.int16:
                rows = rows.view(np.uint16)
            assert rows.ndim == 2 and rows.dtype in (np.uint8, np.uint16)
            n, stride = rows.shape
            v = BatchView()
            v.rows, v.char_width, v.n_rows, v.row_stride, v.row_len = rows.ctypes.data, rows.dtype.itemsize, n, stride, stride
            if lengths is not None:
                lengths = np.ascontiguousarray(lengths, dtype=np.uint32)
                v.lengths = lengths.ctypes.data
            counts = np.zeros(n, dtype=np.uint32)
            st = np.full((n, max_per_row), -1, dtype=np.int32)
            en = np.full((n, max_per_row), -1, dtype=np.int32)
            more = ctypes.c_int(0)
            _check(L.needle_find_all_host(self._h, ctypes.byref(v), int(max_per_row), counts.ctypes.data, st.ctypes.data,
                                          en.ctypes.data, ctypes.byref(more)))
            return counts, st, en, bool(more.value)
        import torch
        assert isinstance(rows, torch.Tensor) and rows.is_cuda and rows.dim() == 2 and rows.is_contiguous()
        v = BatchView()
        n, stride = rows.shape
        v.rows, v.char_width, v.n_rows, v.row_stride, v.row_len = rows.data_ptr(), rows.element_size(), n, stride, stride
        if lengths is not None:
            assert lengths.is_cuda and lengths.dtype == torch.int32 and lengths.shape == (n,)
            v.lengths = lengths.data_ptr()
        with torch.cuda.device(rows.device):
            s = torch.cuda.current_stream(rows.device).cuda_stream if stream is None else stream
            if out is not None:
                counts, st, en = out
                assert counts.shape == (n,) and st.shape == (n, max_per_row) and en.shape == (n, max_per_row)
                assert all(t.is_cuda and t.dtype == torch.int32 and t.is_contiguous() for t in out)
            else:
                counts = torch.zeros(n, dtype=torch.int32, device=rows.device)
                st = torch.full((n, max_per_row), -1, dtype=torch.int32, device=rows.device)
                en = torch.full((n, max_per_row), -1, dtype=torch.int32, device=rows.device)
            more = ctypes.c_int(0)
            _check(L.needle_find_all_dev(self._h, ctypes.byref(v), int(max_per_row), counts.data_ptr(), st.data_ptr(),
                                         en.data_ptr(), ctypes.byref(more), s))
        return counts, st, en, bool(more.value)

    def find_all_dense_packed16(self, rows, max_per_row, lengths=None, stream=None, out=None, want_more=True):
        """needle_find_all_packed16_dev: as find_all_dense on device rows of at most 65 535 chars, each match one dword
        (start | end << 16).  -> (counts int32[n], start_end16 int32[n, max_per_row] (bit pattern of the uint32), more: bool or
        None when want_more is False -- the call is then asynchronous on the stream)."""
        L = _lib.lib()
        if isinstance(rows, np.ndarray):  # host buffers: needle_find_all_packed16_host
            rows = np.ascontiguousarray(rows)
            if rows.dtype == np.int16:
                rows = rows.view(np.uint16)
            assert rows.ndim == 2 and rows.dtype in (np.uint8, np.uint16)
            n, stride = rows.shape
            v = BatchView()
            v.rows, v.char_width, v.n_rows, v.row_stride, v.row_len = rows.ctypes.data, rows.dtype.itemsize, n, stride, stride
            if lengths is not None:
                lengths = np.ascontiguousarray(lengths, dtype=np.uint32)
                v.lengths = lengths.ctypes.data
            counts = np.zeros(n, dtype=np.uint32)
            se = np.full((n, max_per_row), 0xFFFFFFFF, dtype=np.uint32)
            more = ctypes.c_int(0)
            _check(L.needle_find_all_packed16_host(self._h, ctypes.byref(v), int(max_per_row), counts.ctypes.data, se.ctypes.data, ctypes.byref(more)))
            return counts, se, bool(more.value)
        import torch
        v, n = self._dev_view(rows, lengths), rows.shape[0]
        with torch.cuda.device(rows.device):
            s = torch.cuda.current_stream(rows.device).cuda_stream if stream is None else stream
            if out is not None:
                counts, se = out
                assert counts.shape == (n,) and se.shape == (n, max_per_row)
                assert all(t.is_cuda and t.dtype == torch.int32 and t.is_contiguous() for t in out)
            else:
                counts = torch.zeros(n, dtype=torch.int32, device=rows.device)
                se = torch.full((n, max_per_row), -1, dtype=torch.int32, device=rows.device)
            more = ctypes.c_int(0)
            _check(L.needle_find_all_packed16_dev(self._h, ctypes.byref(v), int(max_per_row), counts.data_ptr(), se.data_ptr(),
                                                  ctypes.byref(more) if want_more else None, s))
        return counts, se, (bool(more.value) if want_more else None)

    def find_all_blocked16(self, rows, max_per_row, lengths=None, stream=None, out=None, want_more=True):
        """needle_find_all_blocked16_dev: find_all_dense_packed16 with GROUP-BLOCKED slots -- match k of row r at
        blocks[r >> 6, k, r & 63].  -> (counts int32[n], blocks int32[ceil(n / 64), max_per_row, 64], more)
        (unblock16(blocks, n) gives the [n, max_per_row] view of find_all_dense_packed16)."""
        import torch
        L = _lib.lib()
        v, n = self._dev_view(rows, lengths), rows.shape[0]
        ng = (n + 63) // 64
        with torch.cuda.device(rows.device):
            s = torch.cuda.current_stream(rows.device).cuda_stream if stream is None else stream
            if out is not None:
                counts, blocks = out
                assert counts.shape == (n,) and blocks.shape == (ng, max_per_row, 64)
                assert all(t.is_cuda and t.dtype == torch.int32 and t.is_contiguous() for t in out)
            else:
                counts = torch.zeros(n, dtype=torch.int32, device=rows.device)
                blocks = torch.full((ng, max_per_row, 64), -1, dtype=torch.int32, device=rows.device)
            more = ctypes.c_int(0)
            _check(L.needle_find_all_blocked16_dev(self._h, ctypes.byref(v), int(max_per_row), counts.data_ptr(), blocks.data_ptr(),
                                                   ctypes.byref(more) if want_more else None, s))
        return counts, blocks, (bool(more.value) if want_more else None)

    def find_all_compact16(self, rows, max_per_row=32, lengths=None, stream=None, cap=None, want_more=True):
        """needle_find_all_compact16_dev: every match of every row in compact (CSR) form in ONE call that walks the text once
        -> (offsets int64[n + 1], start_end16 int32[total] (start | end << 16), more: bool or None).  cap: dwords of room for the matches
        (default: 8 per row, grown to the exact total when that was too little); more = some row had more than max_per_row matches (its
        list is cut: raise max_per_row, or use find_all_csr)."""
        import torch
        L = _lib.lib()
        v, n = self._dev_view(rows, lengths), rows.shape[0]
        with torch.cuda.device(rows.device):
            s = torch.cuda.current_stream(rows.device).cuda_stream if stream is None else stream
            offsets = torch.empty(n + 1, dtype=torch.int64, device=rows.device)
            total = torch.zeros(1, dtype=torch.int64, device=rows.device)
            cap = int(cap) if cap is not None else max(1024, 8 * n)
            while True:
                se = torch.empty(cap, dtype=torch.int32, device=rows.device)
                more = ctypes.c_int(0)
                _check(L.needle_find_all_compact16_dev(self._h, ctypes.byref(v), int(max_per_row), offsets.data_ptr(), se.data_ptr(), cap,
                                                       total.data_ptr(), ctypes.byref(more) if want_more else None, s))
                t = int(total.item())
                if t <= cap:
                    return offsets, se[:t], (bool(more.value) if want_more else None)
                cap = t

    @staticmethod
    def unblock16(blocks, n_rows):
        """[groups, slots, 64] group-blocked slots -> [n_rows, slots] row-major (a copy)."""
        g, k, _ = blocks.shape
        return blocks.permute(0, 2, 1).reshape(g * 64, k)[:n_rows].contiguous()

    def _dev_view(self, rows, lengths):
        import torch
        assert isinstance(rows, torch.Tensor) and rows.is_cuda and rows.dim() == 2 and rows.is_contiguous()
        v = BatchView()
        n, stride = rows.shape
        v.rows, v.char_width, v.n_rows, v.row_stride, v.row_len = rows.data_ptr(), rows.element_size(), n, stride, stride
        if lengths is not None:
            assert lengths.is_cuda and lengths.dtype == torch.int32 and lengths.shape == (n,)
            v.lengths = lengths.data_ptr()
        return v

    def count_matches_batch(self, rows, lengths=None, stream=None):
        """needle_count_matches_dev: int32[n_rows], the number of non-overlapping matches of every row."""
        import torch
        L = _lib.lib()
        v = self._dev_view(rows, lengths)
        with torch.cuda.device(rows.device):
            s = torch.cuda.current_stream(rows.device).cuda_stream if stream is None else stream
            counts = torch.empty(rows.shape[0], dtype=torch.int32, device=rows.device)
            _check(L.needle_count_matches_dev(self._h, ctypes.byref(v), counts.data_ptr(), s))
        return counts

    def find_all_csr(self, rows, lengths=None, stream=None):
        """Every non-overlapping match of every row in compact form, two passes over the batch: count
        (needle_count_matches_dev), exclusive prefix sum, fill (needle_find_all_csr_dev).
        -> (offsets int64[n_rows + 1], start int32[m], end int32[m])"""
        L = _lib.lib()
        if isinstance(rows, np.ndarray):  # host buffers: needle_find_all_csr_host (first with a guessed capacity)
            rows = np.ascontiguousarray(rows)
            if rows.dtype == np.int16:
                rows = rows.view(np.uint16)
            assert rows.ndim == 2 and rows.dtype in (np.uint8, np.uint16)
            n, stride = rows.shape
            v = BatchView()
            v.rows, v.char_width, v.n_rows, v.row_stride, v.row_len = rows.ctypes.data, rows.dtype.itemsize, n, stride, stride
            if lengths is not None:
                lengths = np.ascontiguousarray(lengths, dtype=np.uint32)
                v.lengths = lengths.ctypes.data
            offsets = np.zeros(n + 1, dtype=np.uint64)
            capacity = max(1024, 2 * n)
            while True:
                st = np.empty(capacity, dtype=np.int32)
                en = np.empty(capacity, dtype=np.int32)
                total = ctypes.c_uint64(0)
                _check(L.needle_find_all_csr_host(self._h, ctypes.byref(v), offsets.ctypes.data, st.ctypes.data, en.ctypes.data, capacity,
                                                  ctypes.byref(total)))
                if total.value <= capacity:
                    return offsets.astype(np.int64), st[:total.value], en[:total.value]
                capacity = int(total.value)
        import torch
        v = self._dev_view(rows, lengths)
        n = rows.shape[0]
        # the count pass, the prefix sum (torch) and the fill pass all run on ONE stream: a caller-supplied raw stream is made
        # torch's current stream for the torch ops in between (else the cumsum could read counts the count kernel has not
        # written yet, and the fill pass offsets the cumsum has not)
        dev = rows.device
        one = torch.cuda.current_stream(dev) if stream is None else torch.cuda.ExternalStream(stream, device=dev)
        with torch.cuda.device(dev), torch.cuda.stream(one):
            s = one.cuda_stream
            counts = self.count_matches_batch(rows, lengths, s)
            offsets = torch.zeros(n + 1, dtype=torch.int64, device=rows.device)
            torch.cumsum(counts, 0, out=offsets[1:])
            total = int(offsets[-1].item())
            st = torch.empty(total, dtype=torch.int32, device=rows.device)
            en = torch.empty(total, dtype=torch.int32, device=rows.device)
            if total == 0:
                return offsets, st, en
            more = ctypes.c_int(0)
            _check(L.needle_find_all_csr_dev(self._h, ctypes.byref(v), offsets.data_ptr(), st.data_ptr(), en.data_ptr(), ctypes.byref(more), s))
            assert not more.value, "count pass and fill pass disagree"
        return offsets, st, en

    def find_all_batch(self, rows, lengths=None, max_rounds=None):
        """Every non-overlapping match of every row, as the reference's repeated find() would report them
        (DFACompilerTest.java:66-78,671-699) -> (offsets int64[n_rows + 1], start int32[m], end int32[m]) in CSR form:
        find_all_csr (count pass, prefix sum, fill pass); with max_rounds, or for rows of 64 MiB and more, one
        find_next launch per round over the rows that still have a cursor.
        A row ends where the reference's cursor stops advancing: an EMPTY match (or any match that does not end beyond
        the cursor it was searched from) is reported once and ends its row; a nullable pattern's wrapped pseudo-match
        at cursor == length (start = length, end = 0), on which the reference would cycle for ever, is dropped."""
        import torch
        n = rows.shape[0]
        dev = rows.device
        if max_rounds is None and rows.shape[1] * rows.element_size() < (1 << 26):  # count, prefix sum, fill: two passes
            return self.find_all_csr(rows, lengths)
        cursor = torch.zeros(n, dtype=torch.int32, device=dev)
        ids = torch.arange(n, dtype=torch.int64, device=dev)
        counts = torch.zeros(n, dtype=torch.int64, device=dev)
        per_round = []  # round k holds the k-th match of every row that has one: no sort needed to build the CSR
        round_cap = rows.shape[1] + 1  # a row of L chars has at most L non-empty matches (+ one empty one)
        while len(per_round) < round_cap:
            _, st, en = self.find_next_batch(rows, cursor, lengths)
            # en < st: the reference's wrapped pseudo-match of a nullable pattern searched from cursor == length
            # (end = the literal 0 of DFAClassBuilder.java:356); dropped, it ends the row (see needle_find_all_dev)
            hit = (en >= 0) & (en >= st) & (cursor >= 0)
            if not bool(hit.any()):
                break
            per_round.append((ids[hit], st[hit], en[hit]))
            counts += hit
            stop = (en == st) | (en <= cursor)  # the row goes on only while the cursor advances
            cursor = torch.where(hit & ~stop, en, torch.full_like(en, -1))
            if max_rounds is not None and len(per_round) >= max_rounds:
                break
        offsets = torch.zeros(n + 1, dtype=torch.int64, device=dev)
        offsets[1:] = torch.cumsum(counts, 0)
        total = int(offsets[-1].item())
        out_s = torch.empty(total, dtype=torch.int32, device=dev)
        out_e = torch.empty(total, dtype=torch.int32, device=dev)
        for k, (r, s_, e_) in enumerate(per_round):
            pos = offsets[r] + k
            out_s[pos] = s_
            out_e[pos] = e_
        return offsets, out_s, out_e

    def find_batch(self, rows, lengths=None, stream=None, out=None):
        """(bitmap words, start int32[n], end int32[n]); unmatched rows have start = end = -1.  out: optional
        caller-owned (bitmap int64, start int32, end int32) device tensors."""
        return self._run("find", rows, lengths, stream, out)

    def find_packed16_batch(self, rows, lengths=None, stream=None, out=None):
        """needle_find_packed16_dev: find() on device rows of at most 65 534 chars -> (bitmap words, int32[n] tensor whose
        elements are the dwords start | end << 16, -1 (0xFFFFFFFF) = no match), stored by the scan kernel itself: 4 result bytes
        per row instead of 8.  out: optional caller-owned (bitmap int64, packed int32) device tensors."""
        import torch
        v = self._dev_view(rows, lengths)
        n = rows.shape[0]
        with torch.cuda.device(rows.device):
            s = torch.cuda.current_stream(rows.device).cuda_stream if stream is None else stream
            if out is not None:
                words, se = out
                assert words.dtype == torch.int64 and words.numel() >= (n + 63) // 64 and se.dtype == torch.int32 and se.numel() >= n
            else:
                words = torch.empty((n + 63) // 64, dtype=torch.int64, device=rows.device)
                se = torch.empty(n, dtype=torch.int32, device=rows.device)
            _check(_lib.lib().needle_find_packed16_dev(self._h, ctypes.byref(v), words.data_ptr(), se.data_ptr(), s))
        return words, se

    def find_packed8_batch(self, rows, lengths=None, stream=None, out=None):
        """needle_find_packed8_dev: find() on device rows of at most 256 chars -> (bitmap words, int16[n] tensor whose elements are the
        uint16 start | (end - start) << 8; 0xFFFF = no match, 0xFFFE = the match (0, 256)): 2 result bytes per row.
        out: optional caller-owned (bitmap int64, packed int16) device tensors.  unpack8() decodes."""
        import torch
        v = self._dev_view(rows, lengths)
        n = rows.shape[0]
        with torch.cuda.device(rows.device):
            s = torch.cuda.current_stream(rows.device).cuda_stream if stream is None else stream
            if out is not None:
                words, sl = out
                assert words.dtype == torch.int64 and words.numel() >= (n + 63) // 64 and sl.dtype == torch.int16 and sl.numel() >= n
            else:
                words = torch.empty((n + 63) // 64, dtype=torch.int64, device=rows.device)
                sl = torch.empty(n, dtype=torch.int16, device=rows.device)
            _check(_lib.lib().needle_find_packed8_dev(self._h, ctypes.byref(v), words.data_ptr(), sl.data_ptr(), s))
        return words, sl

    @staticmethod
    def unpack8(sl):
        """uint16 entries of needle_find_packed8_* (numpy array, any integer dtype holding the bit pattern) -> (start, end) int32
        arrays, -1 / -1 where there is no match."""
        x = np.asarray(sl).astype(np.int64) & 0xFFFF
        start = np.where(x == 0xFFFF, -1, np.where(x == 0xFFFE, 0, x & 0xFF))
        end = np.where(x == 0xFFFF, -1, np.where(x == 0xFFFE, 256, (x & 0xFF) + (x >> 8)))
        return start.astype(np.int32), end.astype(np.int32)

    def find_packed8_host(self, rows, lengths=None):
        """needle_find_packed8_host: host rows of at most 256 chars -> (bitmap words, uint16[n]: see find_packed8_batch)."""
        L = _lib.lib()
        rows = np.ascontiguousarray(rows)
        if rows.dtype == np.int16:
            rows = rows.view(np.uint16)
        n, stride = rows.shape
        v = BatchView()
        v.rows, v.char_width, v.n_rows, v.row_stride, v.row_len = rows.ctypes.data, rows.dtype.itemsize, n, stride, stride
        if lengths is not None:
            lengths = np.ascontiguousarray(lengths, dtype=np.uint32)
            v.lengths = lengths.ctypes.data
        words = np.zeros((n + 63) // 64, dtype=np.uint64)
        sl = np.zeros(n, dtype=np.uint16)
        _check(L.needle_find_packed8_host(self._h, ctypes.byref(v), words.ctypes.data, sl.ctypes.data))
        return words, sl

    MATCH_REC = np.dtype([("row", np.uint32), ("start", np.uint16), ("end", np.uint16)])  # needle_match_rec

    def find_compact(self, rows, lengths=None, stream=None, out=None):
        """find() with the MATCHED rows only, in row order, as {row u32, start u16, end u16} records
        (needle_find_compact_dev / _host: 8 bytes per matched row instead of 8 per row; rows of at most 65 534 chars).
        Host rows (numpy) -> (bitmap words, records as a MATCH_REC array); device rows (torch) -> (bitmap words,
        records int32[cap, 2] tensor whose rows are the raw records, n_matched as a 1-element int64 device tensor);
        out: optional caller-owned (bitmap int64, records int32[cap, 2], count int64[1]) device tensors."""
        L = _lib.lib()
        if isinstance(rows, np.ndarray):
            rows = np.ascontiguousarray(rows)
            if rows.dtype == np.int16:
                rows = rows.view(np.uint16)
            assert rows.ndim == 2 and rows.dtype in (np.uint8, np.uint16)
            n, stride = rows.shape
            v = BatchView()
            v.rows, v.char_width, v.n_rows, v.row_stride, v.row_len = rows.ctypes.data, rows.dtype.itemsize, n, stride, stride
            if lengths is not None:
                lengths = np.ascontiguousarray(lengths, dtype=np.uint32)
                v.lengths = lengths.ctypes.data
            words = np.zeros((n + 63) // 64, dtype=np.uint64)
            recs = np.zeros(n, dtype=self.MATCH_REC)
            m = ctypes.c_uint64(0)
            _check(L.needle_find_compact_host(self._h, ctypes.byref(v), words.ctypes.data, recs.ctypes.data, n, ctypes.byref(m)))
            return words, recs[:m.value]
        import torch
        v = self._dev_view(rows, lengths)
        n = rows.shape[0]
        with torch.cuda.device(rows.device):
            s = torch.cuda.current_stream(rows.device).cuda_stream if stream is None else stream
            if out is not None:
                words, recs, cnt = out
            else:
                words = torch.empty((n + 63) // 64, dtype=torch.int64, device=rows.device)
                recs = torch.empty((n, 2), dtype=torch.int32, device=rows.device)
                cnt = torch.zeros(1, dtype=torch.int64, device=rows.device)
            _check(L.needle_find_compact_dev(self._h, ctypes.byref(v), words.data_ptr(), recs.data_ptr(), recs.shape[0], cnt.data_ptr(), s))
        return words, recs, cnt

    def find_packed16_host(self, rows, lengths=None):
        """needle_find_packed16_host: host rows -> (bitmap words, uint32[n]: low half start, high half end, 0xFFFF = no match)."""
        L = _lib.lib()
        rows = np.ascontiguousarray(rows)
        if rows.dtype == np.int16:
            rows = rows.view(np.uint16)
        n, stride = rows.shape
        v = BatchView()
        v.rows, v.char_width, v.n_rows, v.row_stride, v.row_len = rows.ctypes.data, rows.dtype.itemsize, n, stride, stride
        if lengths is not None:
            lengths = np.ascontiguousarray(lengths, dtype=np.uint32)
            v.lengths = lengths.ctypes.data
        words = np.zeros((n + 63) // 64, dtype=np.uint64)
        se = np.zeros(n, dtype=np.uint32)
        _check(L.needle_find_packed16_host(self._h, ctypes.byref(v), words.ctypes.data, se.ctypes.data))
        return words, se

    # ---- haystacks packed back to back (one char buffer + offsets: what a JNI host gets from a String[])
    def _run_packed_host(self, op, data, offsets, stream=None, out=None):
        L = _lib.lib()
        if not isinstance(data, np.ndarray) and type(data).__module__.startswith("torch") and data.is_cuda:
            return self._run_packed_dev(op, data, offsets, stream, out)
        data = np.ascontiguousarray(data)
        if data.dtype == np.int16:
            data = data.view(np.uint16)
        assert data.ndim == 1 and data.dtype in (np.uint8, np.uint16), "data: 1-D uint8/uint16 code units"
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        n = offsets.size - 1
        v = _lib.PackedView()
        v.data, v.char_width, v.n_rows, v.offsets = data.ctypes.data, data.dtype.itemsize, n, offsets.ctypes.data
        words = np.zeros((n + 63) // 64, dtype=np.uint64)
        if op == "find":
            st = np.full(n, -1, dtype=np.int32)
            en = np.full(n, -1, dtype=np.int32)
            _check(L.needle_find_packed_host(self._h, ctypes.byref(v), words.ctypes.data, st.ctypes.data, en.ctypes.data))
            return words, st, en
        fn = L.needle_matches_packed_host if op == "matches" else L.needle_contained_in_packed_host
        _check(fn(self._h, ctypes.byref(v), words.ctypes.data))
        return words

    def _run_packed_dev(self, op, data, offsets, stream, out):
        """Device tensors: needle_*_packed_dev -- the packed rows scanned as they lie, results as device tensors."""
        import torch
        L = _lib.lib()
        assert data.dim() == 1 and data.is_contiguous() and data.dtype in (torch.uint8, torch.int16, torch.uint16), \
            "data: 1-D uint8 or (u)int16 code units"
        assert isinstance(offsets, torch.Tensor) and offsets.is_cuda and offsets.device == data.device, "offsets: on data's device"
        assert offsets.dtype == torch.int64 and offsets.dim() == 1 and offsets.is_contiguous() and offsets.numel() >= 1, \
            "offsets: 1-D int64, n + 1 entries"
        n = offsets.numel() - 1
        v = _lib.PackedView()
        v.data, v.char_width, v.n_rows, v.offsets = data.data_ptr(), data.element_size(), n, offsets.data_ptr()
        with torch.cuda.device(data.device):
            s = torch.cuda.current_stream(data.device).cuda_stream if stream is None else stream
            if out is not None:  # caller-owned result buffers (at least as large as the results)
                words = out[0] if isinstance(out, (tuple, list)) else out
                assert words.is_cuda and words.dtype == torch.int64 and words.numel() >= (n + 63) // 64
            else:
                words = torch.empty((n + 63) // 64, dtype=torch.int64, device=data.device)
            if op == "find":
                if out is not None:
                    st, en = out[1], out[2]
                    assert st.dtype == torch.int32 and en.dtype == torch.int32 and st.numel() >= n and en.numel() >= n
                else:
                    st = torch.empty(n, dtype=torch.int32, device=data.device)
                    en = torch.empty(n, dtype=torch.int32, device=data.device)
                _check(L.needle_find_packed_dev(self._h, ctypes.byref(v), words.data_ptr(), st.data_ptr(), en.data_ptr(), s))
                return words, st, en
            fn = L.needle_matches_packed_dev if op == "matches" else L.needle_contained_in_packed_dev
            _check(fn(self._h, ctypes.byref(v), words.data_ptr(), s))
            return words

    def matches_packed(self, data, offsets, stream=None, out=None):
        """matches() of every packed row: numpy data + offsets -> host path (upload, run, download); device tensors (1-D uint8 |
        (u)int16 data, int64 offsets[n + 1]) -> needle_matches_packed_dev, bitmap words as a device tensor.  stream / out: as
        matches_batch (device tensors only)."""
        return self._run_packed_host("matches", data, offsets, stream, out)

    def contained_in_packed(self, data, offsets, stream=None, out=None):
        """Bitmap words of containedIn() of every packed row.  Device tensors (needle_contained_in_packed_dev): patterns with an n-gram
        candidate filter run behind it on packed rows too (set_prefilter / prefilter_state apply as to the fixed-stride calls)."""
        return self._run_packed_host("contained_in", data, offsets, stream, out)

    def find_packed(self, data, offsets, stream=None, out=None):
        """(bitmap words, start, end) of every packed row; device tensors give device tensors (needle_find_packed_dev).  Patterns with an
        n-gram candidate filter and bounded match lengths run behind it (needle_ngram_packed.h; set_prefilter / prefilter_state apply as to
        the fixed-stride calls, PREFILTER_OFF = the plain packed kernel); rows of any length, exact int32 positions."""
        return self._run_packed_host("find", data, offsets, stream, out)

    def find_strings(self, strings):
        """find() over a list of str (UTF-16 code units, like java.lang.String) -> (matched bool[n], start, end)."""
        data, offsets = pack_strings(strings)
        words, st, en = self.find_packed(data, offsets)
        return unpack_bitmap(words, len(strings)), st, en

    def find_next_packed(self, data, offsets, cursor, stream=None):
        """needle_find_next_packed_dev: one find() step per packed row from cursor[r] (device int32[n_rows]; < 0 = row exhausted) ->
        (bitmap words, start, end) device tensors, positions relative to the row -- as find_next_batch on the same rows at a fixed
        stride.  Feeding `end` back as the next cursor enumerates every row's matches."""
        import torch
        L = _lib.lib()
        v = self._packed_dev_view(data, offsets)
        n = v.n_rows
        assert isinstance(cursor, torch.Tensor) and cursor.is_cuda and cursor.dtype == torch.int32 and cursor.is_contiguous() and \
            cursor.numel() >= n, "cursor: device int32[n_rows]"
        with torch.cuda.device(data.device):
            s = torch.cuda.current_stream(data.device).cuda_stream if stream is None else stream
            words = torch.empty((n + 63) // 64, dtype=torch.int64, device=data.device)
            st = torch.empty(n, dtype=torch.int32, device=data.device)
            en = torch.empty(n, dtype=torch.int32, device=data.device)
            _check(L.needle_find_next_packed_dev(self._h, ctypes.byref(v), cursor.data_ptr(), words.data_ptr(), st.data_ptr(), en.data_ptr(), s))
        return words, st, en

    def _find_compact_packed(self, bits, data, offsets, stream, out):
        """find_packed16_packed / find_packed8_packed (bits 16 | 8)."""
        L = _lib.lib()
        rb = np.uint32 if bits == 16 else np.uint16
        if isinstance(data, np.ndarray):  # host buffers: needle_find_packed{16,8}_packed_host
            data = np.ascontiguousarray(data)
            if data.dtype == np.int16:
                data = data.view(np.uint16)
            assert data.ndim == 1 and data.dtype in (np.uint8, np.uint16), "data: 1-D uint8/uint16 code units"
            offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
            n = offsets.size - 1
            v = _lib.PackedView()
            v.data, v.char_width, v.n_rows, v.offsets = data.ctypes.data, data.dtype.itemsize, n, offsets.ctypes.data
            words = np.zeros((n + 63) // 64, dtype=np.uint64)
            res = np.zeros(n, dtype=rb)
            fn = L.needle_find_packed16_packed_host if bits == 16 else L.needle_find_packed8_packed_host
            _check(fn(self._h, ctypes.byref(v), words.ctypes.data, res.ctypes.data))
            return words, res
        import torch
        v = self._packed_dev_view(data, offsets)
        n = v.n_rows
        tdt = torch.int32 if bits == 16 else torch.int16
        with torch.cuda.device(data.device):
            s = torch.cuda.current_stream(data.device).cuda_stream if stream is None else stream
            if out is not None:  # caller-owned (bitmap int64, results int32 | int16, overflow int32 -- zeroed by the caller)
                words, res, ovf = out
                assert words.is_cuda and words.dtype == torch.int64 and words.numel() >= (n + 63) // 64
                assert res.dtype == tdt and res.numel() >= n and ovf.dtype == torch.int32 and ovf.numel() >= 1
            else:
                words = torch.empty((n + 63) // 64, dtype=torch.int64, device=data.device)
                res = torch.empty(n, dtype=tdt, device=data.device)
                ovf = torch.zeros(1, dtype=torch.int32, device=data.device)
            fn = L.needle_find_packed16_packed_dev if bits == 16 else L.needle_find_packed8_packed_dev
            _check(fn(self._h, ctypes.byref(v), words.data_ptr(), res.data_ptr(), ovf.data_ptr(), s))
        return words, res, ovf

    def find_packed16_packed(self, data, offsets, stream=None, out=None):
        """find() of every packed row as ONE dword, start | end << 16 (0xFFFFFFFF = no match; NEEDLE_PACK16_OVER = a match ending past
        65 534).  Device tensors: needle_find_packed16_packed_dev -> (bitmap words, int32[n], overflow int32[1]: 1 when some row
        escaped); out: optional caller-owned (bitmap, results, zeroed overflow) tensors.  Numpy arrays: needle_find_packed16_packed_host
        (rows of at most 65 534 chars) -> (bitmap words, uint32[n]).  unpack16_packed() decodes.  The device form takes the n-gram
        candidate filter as find_packed does, with the same escapes and flag."""
        return self._find_compact_packed(16, data, offsets, stream, out)

    def find_packed8_packed(self, data, offsets, stream=None, out=None):
        """find() of every packed row as ONE uint16, pack8's form (start | (end - start) << 8, 0xFFFF = no match, 0xFFFE = (0, 256);
        NEEDLE_PACK8_OVER = a match ending past 256).  Results as find_packed16_packed (int16 / uint16); the host form takes rows of
        at most 256 chars.  unpack8_packed() decodes.  The device form takes the n-gram candidate filter as find_packed does."""
        return self._find_compact_packed(8, data, offsets, stream, out)

    @staticmethod
    def unpack16_packed(x):
        """Entries of find_packed16_packed (any integer dtype holding the bit pattern) -> (start, end, over) numpy arrays: -1 / -1 where
        there is no match or the match escaped the form (over = True)."""
        x = np.asarray(x).astype(np.int64) & 0xFFFFFFFF
        over = x == PACK16_OVER
        none = (x == 0xFFFFFFFF) | over
        start = np.where(none, -1, x & 0xFFFF)
        end = np.where(none, -1, x >> 16)
        return start.astype(np.int32), end.astype(np.int32), over

    @staticmethod
    def unpack8_packed(x):
        """Entries of find_packed8_packed -> (start, end, over) numpy arrays, pack8's escapes decoded as unpack8; -1 / -1 where there
        is no match or the match escaped the form (over = True)."""
        x = np.asarray(x).astype(np.int64) & 0xFFFF
        over = x == PACK8_OVER
        start, end = Pattern.unpack8(np.where(over, 0xFFFF, x))
        return start, end, over

    # ---- every match of every packed row (needle_*_packed_dev of find-all)
    def _packed_dev_view(self, data, offsets):
        import torch
        assert data.dim() == 1 and data.is_contiguous() and data.dtype in (torch.uint8, torch.int16, torch.uint16), \
            "data: 1-D uint8 or (u)int16 code units"
        assert isinstance(offsets, torch.Tensor) and offsets.is_cuda and offsets.device == data.device, "offsets: on data's device"
        assert offsets.dtype == torch.int64 and offsets.dim() == 1 and offsets.is_contiguous() and offsets.numel() >= 1, \
            "offsets: 1-D int64, n + 1 entries"
        v = _lib.PackedView()
        v.data, v.char_width, v.n_rows, v.offsets = data.data_ptr(), data.element_size(), offsets.numel() - 1, offsets.data_ptr()
        return v

    def count_matches_packed(self, data, offsets, stream=None):
        """needle_count_matches_packed_dev: int32[n_rows], the number of non-overlapping matches of every packed row (device tensors:
        1-D uint8 | (u)int16 data, int64 offsets[n + 1])."""
        import torch
        L = _lib.lib()
        v = self._packed_dev_view(data, offsets)
        with torch.cuda.device(data.device):
            s = torch.cuda.current_stream(data.device).cuda_stream if stream is None else stream
            counts = torch.empty(v.n_rows, dtype=torch.int32, device=data.device)
            _check(L.needle_count_matches_packed_dev(self._h, ctypes.byref(v), counts.data_ptr(), s))
        return counts

    def find_all_packed(self, data, offsets, stream=None):
        """Every non-overlapping match of every packed row in compact form -> (offsets int64[n_rows + 1], start int32[m], end int32[m]).
        numpy data + offsets: needle_find_all_csr_packed_host.  Device tensors: count (needle_count_matches_packed_dev), torch cumsum,
        fill (needle_find_all_csr_packed_dev), all on one stream -- as find_all_csr."""
        L = _lib.lib()
        if isinstance(data, np.ndarray) or not (type(data).__module__.startswith("torch") and data.is_cuda):
            data = np.ascontiguousarray(data)
            if data.dtype == np.int16:
                data = data.view(np.uint16)
            assert data.ndim == 1 and data.dtype in (np.uint8, np.uint16), "data: 1-D uint8/uint16 code units"
            offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
            n = offsets.size - 1
            v = _lib.PackedView()
            v.data, v.char_width, v.n_rows, v.offsets = data.ctypes.data, data.dtype.itemsize, n, offsets.ctypes.data
            out = np.zeros(n + 1, dtype=np.uint64)
            capacity = max(1024, 2 * n)
            while True:  # (first with a guessed capacity, then with the exact total)
                st = np.empty(capacity, dtype=np.int32)
                en = np.empty(capacity, dtype=np.int32)
                total = ctypes.c_uint64(0)
                _check(L.needle_find_all_csr_packed_host(self._h, ctypes.byref(v), out.ctypes.data, st.ctypes.data, en.ctypes.data, capacity,
                                                         ctypes.byref(total)))
                if total.value <= capacity:
                    return out.astype(np.int64), st[:total.value], en[:total.value]
                capacity = int(total.value)
        import torch
        v = self._packed_dev_view(data, offsets)
        n, dev = v.n_rows, data.device
        one = torch.cuda.current_stream(dev) if stream is None else torch.cuda.ExternalStream(stream, device=dev)
        with torch.cuda.device(dev), torch.cuda.stream(one):
            s = one.cuda_stream
            counts = self.count_matches_packed(data, offsets, s)
            out = torch.zeros(n + 1, dtype=torch.int64, device=dev)
            torch.cumsum(counts, 0, out=out[1:])
            total = int(out[-1].item())
            st = torch.empty(total, dtype=torch.int32, device=dev)
            en = torch.empty(total, dtype=torch.int32, device=dev)
            if total == 0:
                return out, st, en
            more = ctypes.c_int(0)
            _check(L.needle_find_all_csr_packed_dev(self._h, ctypes.byref(v), out.data_ptr(), st.data_ptr(), en.data_ptr(), ctypes.byref(more), s))
            assert not more.value, "count pass and fill pass disagree"
        return out, st, en

    def find_all_compact16_packed(self, data, offsets, max_per_row=32, stream=None, cap=None, want_more=True):
        """needle_find_all_compact16_packed_dev (device tensors): every match of every packed row in ONE walk of the text -> (offsets
        int64[n + 1], start_end16 int32[total] (start | end << 16), more: bool or None), as find_all_compact16.  Patterns without a
        find-all transducer raise (use find_all_packed)."""
        import torch
        L = _lib.lib()
        v = self._packed_dev_view(data, offsets)
        n, dev = v.n_rows, data.device
        with torch.cuda.device(dev):
            s = torch.cuda.current_stream(dev).cuda_stream if stream is None else stream
            out = torch.zeros(n + 1, dtype=torch.int64, device=dev)
            total = torch.zeros(1, dtype=torch.int64, device=dev)
            cap = int(cap) if cap is not None else max(1024, 8 * n)
            while True:
                se = torch.empty(cap, dtype=torch.int32, device=dev)
                more = ctypes.c_int(0)
                _check(L.needle_find_all_compact16_packed_dev(self._h, ctypes.byref(v), int(max_per_row), out.data_ptr(), se.data_ptr(), cap,
                                                              total.data_ptr(), ctypes.byref(more) if want_more else None, s))
                t = int(total.item()) if n else 0
                if t <= cap:
                    return out, se[:t], (bool(more.value) if want_more else None)
                cap = t

    def find_all_strings(self, strings):
        """Every non-overlapping match of every str (UTF-16 code units, like java.lang.String) -> list of [(start, end), ...] per string
        (the find_strings counterpart: pack_strings + find_all_packed)."""
        data, offsets = pack_strings(strings)
        off, st, en = self.find_all_packed(data, offsets)
        return [list(zip(st[off[i]:off[i + 1]].tolist(), en[off[i]:off[i + 1]].tolist())) for i in range(len(strings))]

    # ---- replace every match of every packed row (needle_replace_all_*_packed_dev / needle_replace_all_packed_host)
    @staticmethod
    def _repl_units(repl, char_width):
        """The replacement as code units of the rows' width: a str (UTF-16 code units; for 8-bit rows every char must be below 256) or a
        1-D array of code units.  It is literal: no group references."""
        dt = np.uint8 if char_width == 1 else np.uint16
        u = _utf16(repl) if isinstance(repl, str) else np.ascontiguousarray(repl)
        assert u.ndim == 1, "repl: str or 1-D array of code units"
        if u.size and (int(u.min()) < 0 or int(u.max()) > (255 if char_width == 1 else 65535)):
            raise ValueError("replacement holds a code unit that %d-byte rows cannot hold" % char_width)
        if u.size > _lib.REPLACE_MAX_UNITS:
            raise ValueError("replacement longer than %d code units" % _lib.REPLACE_MAX_UNITS)
        return np.ascontiguousarray(u.astype(dt))

    @staticmethod
    def splice_packed(data, offsets, match_offsets, start, end, repl, stream=None, out=None, out_start=0):
        """The two pattern-free entries (needle_replace_all_lengths_packed_dev, torch cumsum, needle_replace_all_fill_packed_dev) on one
        stream: every match of the caller's CSR list (match_offsets int64[n + 1], start / end int32, positions relative to the row,
        monotone within each row -- find_all_packed's result, or a subset of it) replaced by `repl` -> (out_data, out_offsets int64[n + 1]).
        out: optional caller-owned tensor of the rows' dtype; the result then starts at its code unit out_start (appending) and out_offsets
        are positions in `out`; units outside [out_offsets[0], out_offsets[n]) are left as they are.  The one host read is the total.
        numpy inputs are uploaded, spliced on the device and brought back."""
        import torch
        L = _lib.lib()
        if isinstance(data, np.ndarray):
            data = np.ascontiguousarray(data)
            if data.dtype == np.uint16:
                data = data.view(np.int16)
            dev = lambda x, dt: torch.from_numpy(np.ascontiguousarray(x).astype(dt)).to("cuda")
            o, oo = Pattern.splice_packed(dev(np.concatenate([data, np.zeros((-data.nbytes) % 4 // data.itemsize, data.dtype)]), data.dtype),
                                          dev(offsets, np.int64), dev(match_offsets, np.int64), dev(start, np.int32), dev(end, np.int32), repl, stream)
            o = o.cpu().numpy()
            return (o.view(np.uint16) if o.dtype == np.int16 else o), oo.cpu().numpy()
        assert data.dim() == 1 and data.is_contiguous() and data.dtype in (torch.uint8, torch.int16, torch.uint16), "data: 1-D uint8 or (u)int16 code units"
        for t, dt, what in ((offsets, torch.int64, "offsets"), (match_offsets, torch.int64, "match_offsets"), (start, torch.int32, "start"), (end, torch.int32, "end")):
            assert isinstance(t, torch.Tensor) and t.device == data.device and t.dtype == dt and t.dim() == 1 and t.is_contiguous(), what
        n, dv, cw = offsets.numel() - 1, data.device, data.element_size()
        assert n >= 0 and match_offsets.numel() == n + 1 and start.numel() == end.numel()
        r = Pattern._repl_units(repl, cw)
        v = _lib.PackedView()
        v.data, v.char_width, v.n_rows, v.offsets = data.data_ptr(), cw, n, offsets.data_ptr()
        one = torch.cuda.current_stream(dv) if stream is None else torch.cuda.ExternalStream(stream, device=dv)
        with torch.cuda.device(dv), torch.cuda.stream(one):
            s = one.cuda_stream
            sp, ep = (start.data_ptr(), end.data_ptr()) if start.numel() else (None, None)
            lens = torch.empty(n, dtype=torch.int64, device=dv)
            _check(L.needle_replace_all_lengths_packed_dev(ctypes.byref(v), match_offsets.data_ptr(), sp, ep, r.size, lens.data_ptr(), s))
            out_off = torch.full((n + 1,), int(out_start), dtype=torch.int64, device=dv)
            if n:
                out_off[1:] += torch.cumsum(lens, 0)
            total = int(out_off[-1].item())
            if out is None:
                room = torch.empty(total + 4, dtype=data.dtype, device=dv)  # (never an empty allocation: its pointer would be NULL)
                out = room[:total]
            else:
                assert out.device == dv and out.dtype == data.dtype and out.dim() == 1 and out.is_contiguous() and out.numel() >= total
                room = out
            _check(L.needle_replace_all_fill_packed_dev(ctypes.byref(v), match_offsets.data_ptr(), sp, ep, r.ctypes.data if r.size else None, r.size,
                                                        out_off.data_ptr(), room.data_ptr(), s))  # (an empty view's pointer is NULL too: a result of no units)
        return out, out_off

    @staticmethod
    def _repl_table(repls, char_width):
        """A replacement table (a list of str or 1-D arrays, each through _repl_units) -> (its code units back to back, uint32
        offsets[len + 1]).  ValueError: no entry, more than 256 entries, more than 4096 code units in all."""
        repls = list(repls)
        if not 1 <= len(repls) <= _lib.REPLACE_MAX_CHOICES:
            raise ValueError("a replacement table holds 1 .. %d entries" % _lib.REPLACE_MAX_CHOICES)
        parts = [Pattern._repl_units(r, char_width) for r in repls]
        off = np.zeros(len(parts) + 1, dtype=np.uint32)
        off[1:] = np.cumsum([u.size for u in parts])
        if int(off[-1]) > _lib.REPLACE_MAX_UNITS:
            raise ValueError("replacement table longer than %d code units" % _lib.REPLACE_MAX_UNITS)
        return np.ascontiguousarray(np.concatenate(parts)), off

    @staticmethod
    def splice_each_packed(data, offsets, match_offsets, start, end, choice, repls, stream=None, out=None, out_start=0, lowest_bit=False):
        """splice_packed with a replacement PER MATCH (needle_replace_each_lengths_packed_dev, torch cumsum,
        needle_replace_each_fill_packed_dev on one stream): match m of the caller's CSR list is replaced by repls[c] when
        0 <= c < len(repls) and KEPT as it is for every other c -> (out_data, out_offsets int64[n + 1]).  choice: int32, indexed like
        start; c = choice[m], or with lowest_bit=True the index of the lowest set bit of the mask choice[m] (-1 for 0) -- what
        PatternSet.matches_spans_packed returns goes in as it is.  repls: a list of str or 1-D arrays of code units (at most 256
        entries, 4096 code units in all).  out / out_start, the one host read and numpy inputs: as splice_packed."""
        import torch
        L = _lib.lib()
        if isinstance(data, np.ndarray):
            data = np.ascontiguousarray(data)
            if data.dtype == np.uint16:
                data = data.view(np.int16)
            dev = lambda x, dt: torch.from_numpy(np.ascontiguousarray(x).astype(dt)).to("cuda")
            ch = np.ascontiguousarray(choice)
            ch = ch.view(np.int32) if ch.dtype == np.uint32 else ch.astype(np.int32)
            o, oo = Pattern.splice_each_packed(dev(np.concatenate([data, np.zeros((-data.nbytes) % 4 // data.itemsize, data.dtype)]), data.dtype),
                                               dev(offsets, np.int64), dev(match_offsets, np.int64), dev(start, np.int32), dev(end, np.int32),
                                               dev(ch, np.int32), repls, stream, lowest_bit=lowest_bit)
            o = o.cpu().numpy()
            return (o.view(np.uint16) if o.dtype == np.int16 else o), oo.cpu().numpy()
        assert data.dim() == 1 and data.is_contiguous() and data.dtype in (torch.uint8, torch.int16, torch.uint16), "data: 1-D uint8 or (u)int16 code units"
        for t, dt, what in ((offsets, torch.int64, "offsets"), (match_offsets, torch.int64, "match_offsets"), (start, torch.int32, "start"),
                            (end, torch.int32, "end"), (choice, torch.int32, "choice")):
            assert isinstance(t, torch.Tensor) and t.device == data.device and t.dtype == dt and t.dim() == 1 and t.is_contiguous(), what
        n, dv, cw = offsets.numel() - 1, data.device, data.element_size()
        assert n >= 0 and match_offsets.numel() == n + 1 and start.numel() == end.numel() == choice.numel()
        r, roff = Pattern._repl_table(repls, cw)
        form = _lib.CHOICE_LOWEST_BIT if lowest_bit else _lib.CHOICE_INDEX
        v = _lib.PackedView()
        v.data, v.char_width, v.n_rows, v.offsets = data.data_ptr(), cw, n, offsets.data_ptr()
        one = torch.cuda.current_stream(dv) if stream is None else torch.cuda.ExternalStream(stream, device=dv)
        with torch.cuda.device(dv), torch.cuda.stream(one):
            s = one.cuda_stream
            sp, ep, cp = (start.data_ptr(), end.data_ptr(), choice.data_ptr()) if start.numel() else (None, None, None)
            lens = torch.empty(n, dtype=torch.int64, device=dv)
            _check(L.needle_replace_each_lengths_packed_dev(ctypes.byref(v), match_offsets.data_ptr(), sp, ep, cp, form, roff.ctypes.data, roff.size - 1,
                                                            lens.data_ptr(), s))
            out_off = torch.full((n + 1,), int(out_start), dtype=torch.int64, device=dv)
            if n:
                out_off[1:] += torch.cumsum(lens, 0)
            total = int(out_off[-1].item())
            if out is None:
                room = torch.empty(total + 4, dtype=data.dtype, device=dv)  # (never an empty allocation: its pointer would be NULL)
                out = room[:total]
            else:
                assert out.device == dv and out.dtype == data.dtype and out.dim() == 1 and out.is_contiguous() and out.numel() >= total
                room = out
            _check(L.needle_replace_each_fill_packed_dev(ctypes.byref(v), match_offsets.data_ptr(), sp, ep, cp, form, r.ctypes.data if r.size else None,
                                                         roff.ctypes.data, roff.size - 1, out_off.data_ptr(), room.data_ptr(), s))
        return out, out_off

    def replace_all_packed(self, data, offsets, repl, stream=None, out=None, out_start=0):
        """Every non-overlapping match of every packed row -- the matches find_all_packed files -- replaced by the literal `repl` (a str, or a
        1-D array of code units) -> (out_data, out_offsets[n + 1]): row r's result is out_data[out_offsets[r]:out_offsets[r + 1]].  What a
        caller gets who loops the reference's find() and appends to a StringBuilder (an empty match is replaced once and ends its row);
        not java.util.regex's replaceAll for nullable patterns.  Device tensors: find_all_packed's count / cumsum / fill, then splice_packed
        (lengths, cumsum, fill), all on one stream; the host reads the two totals.  out / out_start: as splice_packed.  numpy data + offsets:
        needle_replace_all_packed_host."""
        L = _lib.lib()
        if isinstance(data, np.ndarray) or not (type(data).__module__.startswith("torch") and data.is_cuda):
            data = np.ascontiguousarray(data)
            if data.dtype == np.int16:
                data = data.view(np.uint16)
            assert data.ndim == 1 and data.dtype in (np.uint8, np.uint16), "data: 1-D uint8/uint16 code units"
            offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
            n = offsets.size - 1
            r = Pattern._repl_units(repl, data.dtype.itemsize)
            v = _lib.PackedView()
            v.data, v.char_width, v.n_rows, v.offsets = data.ctypes.data, data.dtype.itemsize, n, offsets.ctypes.data
            out_off = np.zeros(n + 1, dtype=np.uint64)
            capacity = max(1024, 2 * int(offsets[-1] - offsets[0]))
            while True:  # (first with a guessed capacity, then with the exact total)
                text = np.empty(capacity, dtype=data.dtype)
                total = ctypes.c_uint64(0)
                _check(L.needle_replace_all_packed_host(self._h, ctypes.byref(v), r.ctypes.data if r.size else None, r.size, out_off.ctypes.data,
                                                        text.ctypes.data, capacity, ctypes.byref(total)))
                if total.value <= capacity:
                    return text[:total.value], out_off.astype(np.int64)
                capacity = int(total.value)
        off, st, en = self.find_all_packed(data, offsets, stream=stream)
        return Pattern.splice_packed(data, offsets, off, st, en, repl, stream=stream, out=out, out_start=out_start)

    def replace_first_packed(self, data, offsets, repl, stream=None, out=None, out_start=0):
        """The first match of every packed row (find_packed's) replaced by `repl` -> (out_data, out_offsets): find_packed's results turned
        into a list of at most one match per row (cumsum of the matched bits), then splice_packed.  numpy inputs are uploaded first."""
        import torch
        if isinstance(data, np.ndarray):
            data = np.ascontiguousarray(data)
            if data.dtype == np.uint16:
                data = data.view(np.int16)
            pad = np.zeros((-data.nbytes) % 4 // data.itemsize, data.dtype)
            o, oo = self.replace_first_packed(torch.from_numpy(np.concatenate([data, pad])).to("cuda"),
                                              torch.from_numpy(np.ascontiguousarray(offsets).astype(np.int64)).to("cuda"), repl, stream)
            o = o.cpu().numpy()
            return (o.view(np.uint16) if o.dtype == np.int16 else o), oo.cpu().numpy()
        dv, n = data.device, offsets.numel() - 1
        one = torch.cuda.current_stream(dv) if stream is None else torch.cuda.ExternalStream(stream, device=dv)
        with torch.cuda.device(dv), torch.cuda.stream(one):
            words, st, en = self.find_packed(data, offsets, stream=stream)
            hit = ((words.unsqueeze(1) >> torch.arange(64, device=dv)) & 1).reshape(-1)[:n].bool()
            moff = torch.zeros(n + 1, dtype=torch.int64, device=dv)
            if n:
                torch.cumsum(hit, 0, out=moff[1:])
            st1, en1 = st[:n][hit].contiguous(), en[:n][hit].contiguous()
        return Pattern.splice_packed(data, offsets, moff, st1, en1, repl, stream=stream, out=out, out_start=out_start)

    def replace_all_strings(self, strings, repl):
        """Every match of every str replaced by the str `repl` -> list[str] (UTF-16 code units, like java.lang.String): pack_strings +
        replace_all_packed, the counterpart of find_all_strings."""
        data, offsets = pack_strings(strings)
        text, off = self.replace_all_packed(data, offsets, repl)
        return [text[off[i]:off[i + 1]].tobytes().decode("utf-16-le", "surrogatepass") for i in range(len(strings))]

    # ---- spans of packed rows as a new packed batch: extract, split, select (needle_gather_spans_*_packed_dev,
    # needle_split_spans_packed_dev, needle_gather_matches_packed_host)
    @staticmethod
    def _gather_host_args(data, arrays):
        """numpy packed data (padded to whole 4 bytes) and int arrays on the device, for the static methods' numpy form."""
        import torch
        data = np.ascontiguousarray(data)
        if data.dtype == np.uint16:
            data = data.view(np.int16)
        pad = np.zeros(4 // data.itemsize + (-data.nbytes) % 4 // data.itemsize, data.dtype)
        up = lambda x, dt: torch.from_numpy(np.ascontiguousarray(x).astype(dt)).to("cuda")
        return up(np.concatenate([data, pad]), data.dtype), [up(x, dt) for x, dt in arrays]

    @staticmethod
    def _gather_host_text(text):
        text = text.cpu().numpy()
        return text.view(np.uint16) if text.dtype == np.int16 else text

    @staticmethod
    def _gather_check(data, tensors):
        import torch
        assert data.dim() == 1 and data.is_contiguous() and data.dtype in (torch.uint8, torch.int16, torch.uint16), "data: 1-D uint8 or (u)int16 code units"
        for t, dt, what in tensors:
            assert isinstance(t, torch.Tensor) and t.device == data.device and t.dtype == dt and t.dim() == 1 and t.is_contiguous(), what

    @staticmethod
    def gather_spans_packed(data, offsets, span_offsets, start, end, stream=None, out=None, out_start=0):
        """The spans of a CSR list over packed rows as a NEW packed batch (needle_gather_spans_lengths_packed_dev, torch cumsum,
        needle_gather_spans_fill_packed_dev on one stream): span m of row r -- span_offsets int64[n + 1], start / end int32, positions
        relative to the row, find_all_packed's result or any list: repeated, overlapping, reversed and out-of-row spans are clamped into
        their row -- gives the output row row_r[s':e'] -> (out_data, out_offsets).  out_offsets is indexed like start, one entry more:
        for a list that fills start / end (span_offsets[0] == 0, span_offsets[n] == len(start)) it is the new batch's offsets as they
        are; entries outside the list repeat their neighbour.  out: optional caller-owned tensor of the rows' dtype; the result then
        starts at its code unit out_start (appending) and out_offsets are positions in `out`; units outside the result are left as they
        are.  The one host read is the total.  numpy inputs are uploaded, gathered on the device and brought back."""
        import torch
        L = _lib.lib()
        if isinstance(data, np.ndarray):
            d, (o, so, st, en) = Pattern._gather_host_args(data, ((offsets, np.int64), (span_offsets, np.int64), (start, np.int32), (end, np.int32)))
            text, oo = Pattern.gather_spans_packed(d, o, so, st, en, stream)
            return Pattern._gather_host_text(text), oo.cpu().numpy()
        Pattern._gather_check(data, ((offsets, torch.int64, "offsets"), (span_offsets, torch.int64, "span_offsets"), (start, torch.int32, "start"),
                                     (end, torch.int32, "end")))
        n, dv, m = offsets.numel() - 1, data.device, start.numel()
        assert n >= 0 and span_offsets.numel() == n + 1 and end.numel() == m
        v = _lib.PackedView()
        v.data, v.char_width, v.n_rows, v.offsets = data.data_ptr(), data.element_size(), n, offsets.data_ptr()
        one = torch.cuda.current_stream(dv) if stream is None else torch.cuda.ExternalStream(stream, device=dv)
        with torch.cuda.device(dv), torch.cuda.stream(one):
            s = one.cuda_stream
            sp, ep = (start.data_ptr(), end.data_ptr()) if m else (None, None)
            lens = torch.zeros(m + 1, dtype=torch.int64, device=dv)  # (entries outside the list stay 0; never an empty allocation)
            _check(L.needle_gather_spans_lengths_packed_dev(ctypes.byref(v), span_offsets.data_ptr(), sp, ep, lens.data_ptr(), s))
            out_off = torch.full((m + 1,), int(out_start), dtype=torch.int64, device=dv)
            if m:
                out_off[1:] += torch.cumsum(lens[:m], 0)
            total = int(out_off[-1].item())
            if out is None:
                room = torch.empty(total + 4, dtype=data.dtype, device=dv)  # (never an empty allocation: its pointer would be NULL)
                out = room[:total]
            else:
                assert out.device == dv and out.dtype == data.dtype and out.dim() == 1 and out.is_contiguous() and out.numel() >= total
                room = out
            if room.numel():  # (an `out` of no units has no address to hand over, and nothing is to be written)
                _check(L.needle_gather_spans_fill_packed_dev(ctypes.byref(v), span_offsets.data_ptr(), sp, ep, out_off.data_ptr(), room.data_ptr(), s))
        return out, out_off

    @staticmethod
    def split_spans_packed(data, offsets, match_offsets, start, end, stream=None):
        """A match list's complement (needle_split_spans_packed_dev): the c matches of a row give c + 1 pieces -- the text in front of the
        first match, between the matches, behind the last; empty pieces are kept -> (piece_offsets int64[n + 1], piece_start int32,
        piece_end int32), a span list for gather_spans_packed.  The one host read is the number of matches.  numpy inputs are uploaded."""
        import torch
        L = _lib.lib()
        if isinstance(data, np.ndarray):
            d, (o, mo, st, en) = Pattern._gather_host_args(data, ((offsets, np.int64), (match_offsets, np.int64), (start, np.int32), (end, np.int32)))
            return tuple(x.cpu().numpy() for x in Pattern.split_spans_packed(d, o, mo, st, en, stream))
        Pattern._gather_check(data, ((offsets, torch.int64, "offsets"), (match_offsets, torch.int64, "match_offsets"), (start, torch.int32, "start"),
                                     (end, torch.int32, "end")))
        n, dv = offsets.numel() - 1, data.device
        assert n >= 0 and match_offsets.numel() == n + 1 and start.numel() == end.numel()
        v = _lib.PackedView()
        v.data, v.char_width, v.n_rows, v.offsets = data.data_ptr(), data.element_size(), n, offsets.data_ptr()
        one = torch.cuda.current_stream(dv) if stream is None else torch.cuda.ExternalStream(stream, device=dv)
        with torch.cuda.device(dv), torch.cuda.stream(one):
            pieces = int((match_offsets[-1] - match_offsets[0]).item()) + n
            po = torch.zeros(n + 1, dtype=torch.int64, device=dv)
            room = torch.empty(2 * pieces + 1, dtype=torch.int32, device=dv)  # (never an empty allocation: its pointer would be NULL)
            sp, ep = (start.data_ptr(), end.data_ptr()) if start.numel() else (None, None)
            _check(L.needle_split_spans_packed_dev(ctypes.byref(v), match_offsets.data_ptr(), sp, ep, po.data_ptr(), room.data_ptr(),
                                                   room.data_ptr() + 4 * pieces, one.cuda_stream))
        return po, room[:pieces], room[pieces:2 * pieces]

    # ---- distinct spans and their counts: equal spans of a list put into groups (needle_group_spans_packed_dev)
    @staticmethod
    def group_spans_packed(data, offsets, span_offsets, start, end, stream=None, hash_bits=64):
        """needle_group_spans_packed_dev: per span of a CSR list over packed rows the FIRST span with the same (clamped) text and the size
        of its group -> (first int64[M], count int32[M]) on the device, indexed like `start`: first[m] is the smallest index whose text
        equals span m's, count[m] the number of such spans.  A span with start < 0 and end < 0 is absent (an unpassed capture group):
        first -1 (NEEDLE_GROUP_NONE), count 0 -- as have the entries outside [span_offsets[0], span_offsets[n]).  The leaders, first[m]
        == m, are the distinct texts in first-occurrence order.  Exact (texts are compared, not hashes) and deterministic.  The
        workspace is sized from start.numel(); the one host read is the status, and status 1 (more spans named by span_offsets than start /
        end hold, or a full table) raises, also for an empty start / end.  hash_bits (0 .. 64) never changes
        the result: fewer bits make different texts share probe chains (tests).  numpy inputs are uploaded and the results brought back."""
        import torch
        L = _lib.lib()
        if isinstance(data, np.ndarray):
            d, (o, so, st, en) = Pattern._gather_host_args(data, ((offsets, np.int64), (span_offsets, np.int64), (start, np.int32), (end, np.int32)))
            return tuple(x.cpu().numpy() for x in Pattern.group_spans_packed(d, o, so, st, en, stream, hash_bits))
        Pattern._gather_check(data, ((offsets, torch.int64, "offsets"), (span_offsets, torch.int64, "span_offsets"), (start, torch.int32, "start"),
                                     (end, torch.int32, "end")))
        n, dv, m = offsets.numel() - 1, data.device, start.numel()
        assert n >= 0 and span_offsets.numel() == n + 1 and end.numel() == m, "span_offsets: n_rows + 1 entries; start / end alike"
        v = _lib.PackedView()
        v.data, v.char_width, v.n_rows, v.offsets = data.data_ptr(), data.element_size(), n, offsets.data_ptr()
        one = torch.cuda.current_stream(dv) if stream is None else torch.cuda.ExternalStream(stream, device=dv)
        with torch.cuda.device(dv), torch.cuda.stream(one):
            first_room = torch.full((m + 1,), -1, dtype=torch.int64, device=dv)  # (never an empty tensor: its pointer would be NULL)
            count_room = torch.zeros(m + 1, dtype=torch.int32, device=dv)
            first, count = first_room[:m], count_room[:m]
            if n == 0:
                return first, count
            work_bytes = int(L.needle_group_spans_work_bytes(m))
            work = torch.empty((work_bytes + 7) // 8, dtype=torch.int64, device=dv)
            status = torch.zeros(1, dtype=torch.int32, device=dv)
            sp, ep = (start.data_ptr(), end.data_ptr()) if m else (None, None)  # (no spans: the status still says whether the offsets agree)
            _check(L.needle_group_spans_packed_dev(ctypes.byref(v), span_offsets.data_ptr(), sp, ep, m, hash_bits,
                                                   work.data_ptr(), work_bytes, first_room.data_ptr(), count_room.data_ptr(), status.data_ptr(),
                                                   one.cuda_stream))
            if int(status.item()) != 0:
                raise DeviceError("needle_group_spans_packed_dev: status 1 -- the span offsets name more spans than start / end hold "
                                  "(max_spans), or the table filled")
        return first, count

    @staticmethod
    def distinct_spans_packed(data, offsets, span_offsets, start, end, stream=None):
        """The distinct texts of a span list and how often each occurs (grep -o | sort | uniq -c without the sort) -> (text, text_offsets,
        counts int32[k], group_of_span int64[M]): distinct text g -- in first-occurrence order -- is text[text_offsets[g]:text_offsets[g +
        1]] and occurs counts[g] times; span m belongs to group_of_span[m] (-1: an absent span, or an entry outside the list).
        group_spans_packed, the leaders by first == arange, group ids by a cumsum over the leaders, the leaders' own CSR list over the
        rows, gather_spans_packed on it: everything stays on the device, and (text, text_offsets) is a packed batch every entry takes.
        numpy inputs are uploaded and the results brought back."""
        import torch
        if isinstance(data, np.ndarray):
            d, (o, so, st, en) = Pattern._gather_host_args(data, ((offsets, np.int64), (span_offsets, np.int64), (start, np.int32), (end, np.int32)))
            text, toff, counts, gid = Pattern.distinct_spans_packed(d, o, so, st, en, stream)
            return Pattern._gather_host_text(text), toff.cpu().numpy(), counts.cpu().numpy(), gid.cpu().numpy()
        first, count = Pattern.group_spans_packed(data, offsets, span_offsets, start, end, stream)
        dv, m = data.device, start.numel()
        one = torch.cuda.current_stream(dv) if stream is None else torch.cuda.ExternalStream(stream, device=dv)
        with torch.cuda.device(dv), torch.cuda.stream(one):
            leader = first == torch.arange(m, dtype=torch.int64, device=dv)
            before = torch.zeros(m + 1, dtype=torch.int64, device=dv)  # leaders in front of entry m
            if m:
                torch.cumsum(leader, 0, out=before[1:])
            gid = torch.where(first >= 0, before[first.clamp(min=0)], torch.full_like(first, -1))
            lso = before[span_offsets.clamp(0, m)]  # the leaders' list over the rows (no leader lies in front of span_offsets[0])
            lst, len_, counts = start[leader].contiguous(), end[leader].contiguous(), count[leader].contiguous()
        text, toff = Pattern.gather_spans_packed(data, offsets, lso, lst, len_, stream=stream)
        return text, toff, counts, gid

    def distinct_matches_packed(self, data, offsets, stream=None):
        """The distinct matches of every packed row and their counts -> (text, text_offsets, counts, group_of_match) as
        distinct_spans_packed, on find_all_packed's list.  numpy inputs are uploaded and the results brought back."""
        if isinstance(data, np.ndarray):
            d, (o,) = Pattern._gather_host_args(data, ((offsets, np.int64),))
            text, toff, counts, gid = self.distinct_matches_packed(d, o, stream)
            return Pattern._gather_host_text(text), toff.cpu().numpy(), counts.cpu().numpy(), gid.cpu().numpy()
        off, st, en = self.find_all_packed(data, offsets, stream=stream)
        return Pattern.distinct_spans_packed(data, offsets, off, st, en, stream=stream)

    @staticmethod
    def _distinct_table(text, toff, counts, decode):
        text, toff, counts = np.asarray(text), np.asarray(toff), np.asarray(counts)
        return [(decode(text[toff[g]:toff[g + 1]]), int(counts[g])) for g in range(counts.size)]

    def count_distinct_strings(self, strings):
        """The distinct matches over all strs and how often each occurs -> list[(str, int)] in first-occurrence order
        (collections.Counter over re.findall, insertion-ordered): pack_strings + distinct_matches_packed."""
        data, offsets = pack_strings(strings)
        text, toff, counts, _ = self.distinct_matches_packed(data, offsets)
        return Pattern._distinct_table(text, toff, counts, lambda u: u.tobytes().decode("utf-16-le", "surrogatepass"))

    def count_distinct_bytes(self, rows):
        """count_distinct_strings for UTF-8 `bytes` rows -> list[(bytes, int)]: find_all_utf8_packed's byte positions, grouped at char
        width 1 on the ORIGINAL bytes -- no encoder back to UTF-8 is involved; matches are equal when their bytes are."""
        data, offsets = pack_bytes(rows)
        d, o, _ = Pattern._utf8_dev(data, offsets)
        moff, bs, be = self.find_all_utf8_packed(d, o)
        text, toff, counts, _ = Pattern.distinct_spans_packed(d, o, moff, bs, be)
        return Pattern._distinct_table(text.cpu().numpy(), toff.cpu().numpy(), counts.cpu().numpy(), lambda u: u.tobytes())

    def count_distinct_group_strings(self, strings, g):
        """The distinct texts of capturing group g over every match of every str -> list[(str, int)] in first-occurrence order (GROUP BY
        regexp_extract(.., g)): plane g of find_all_groups_packed through distinct_spans_packed.  A group the match did not pass is
        absent: it is not reported and counts for nobody."""
        data, offsets = pack_strings(strings)
        d, (o,) = Pattern._gather_host_args(data, ((offsets, np.int64),))
        off, gs, ge = self.find_all_groups_packed(d, o)
        assert 0 <= g < gs.size(0), "group out of range"
        text, toff, counts, _ = Pattern.distinct_spans_packed(d, o, off, gs[g].contiguous(), ge[g].contiguous())
        return Pattern._distinct_table(Pattern._gather_host_text(text), toff.cpu().numpy(), counts.cpu().numpy(),
                                       lambda u: u.tobytes().decode("utf-16-le", "surrogatepass"))

    @staticmethod
    def distinct_rows_packed(data, offsets, stream=None):
        """The distinct rows of a packed batch and their counts (sort -u / uniq -c of lines without the sort) -> (text, text_offsets,
        counts, group_of_row) as distinct_spans_packed, with the list (0, 2^31 - 1) for every row: the clamp makes the span the row."""
        import torch
        if isinstance(data, np.ndarray):
            d, (o,) = Pattern._gather_host_args(data, ((offsets, np.int64),))
            text, toff, counts, gid = Pattern.distinct_rows_packed(d, o, stream)
            return Pattern._gather_host_text(text), toff.cpu().numpy(), counts.cpu().numpy(), gid.cpu().numpy()
        n, dv = offsets.numel() - 1, data.device
        one = torch.cuda.current_stream(dv) if stream is None else torch.cuda.ExternalStream(stream, device=dv)
        with torch.cuda.device(dv), torch.cuda.stream(one):
            so = torch.arange(n + 1, dtype=torch.int64, device=dv)
            st = torch.zeros(n, dtype=torch.int32, device=dv)
            en = torch.full((n,), 0x7FFFFFFF, dtype=torch.int32, device=dv)
        return Pattern.distinct_spans_packed(data, offsets, so, st, en, stream=stream)

    def _gather_matches_host(self, mode, data, offsets):
        """needle_gather_matches_packed_host on numpy data + offsets: first with guessed capacities, then with the exact totals."""
        L = _lib.lib()
        data = np.ascontiguousarray(data)
        if data.dtype == np.int16:
            data = data.view(np.uint16)
        assert data.ndim == 1 and data.dtype in (np.uint8, np.uint16), "data: 1-D uint8/uint16 code units"
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        n = offsets.size - 1
        v = _lib.PackedView()
        v.data, v.char_width, v.n_rows, v.offsets = data.ctypes.data, data.dtype.itemsize, n, offsets.ctypes.data
        span_off = np.zeros(n + 1, dtype=np.uint64)
        span_cap, unit_cap = max(1024, 2 * n), max(1024, int(offsets[-1] - offsets[0]))
        while True:
            out_off = np.zeros(span_cap + 1, dtype=np.uint64)
            text = np.empty(unit_cap, dtype=data.dtype)
            spans, units = ctypes.c_uint64(0), ctypes.c_uint64(0)
            _check(L.needle_gather_matches_packed_host(self._h, ctypes.byref(v), mode, span_off.ctypes.data, out_off.ctypes.data, span_cap,
                                                       text.ctypes.data, unit_cap, ctypes.byref(spans), ctypes.byref(units)))
            if spans.value <= span_cap and units.value <= unit_cap:
                return text[:units.value], out_off[:spans.value + 1].astype(np.int64), span_off.astype(np.int64)
            span_cap, unit_cap = max(span_cap, int(spans.value)), max(unit_cap, int(units.value))

    def extract_all_packed(self, data, offsets, stream=None, out=None, out_start=0):
        """Every non-overlapping match of every packed row -- the matches find_all_packed files -- as the rows of a NEW packed batch (grep
        -o, regexp_extract_all) -> (out_data, out_offsets, span_offsets int64[n + 1]): input row r gave the output rows span_offsets[r] ..
        span_offsets[r + 1], output row m is out_data[out_offsets[m]:out_offsets[m + 1]].  (out_data, out_offsets) goes into every
        *_packed method as it is.  Device tensors: find_all_packed through the pattern's own route, then gather_spans_packed, on one
        stream; out / out_start as gather_spans_packed.  numpy data + offsets: needle_gather_matches_packed_host."""
        if isinstance(data, np.ndarray) or not (type(data).__module__.startswith("torch") and data.is_cuda):
            return self._gather_matches_host(_lib.GATHER_MATCHES, data, offsets)
        off, st, en = self.find_all_packed(data, offsets, stream=stream)
        text, oo = Pattern.gather_spans_packed(data, offsets, off, st, en, stream=stream, out=out, out_start=out_start)
        return text, oo, off

    def split_packed(self, data, offsets, stream=None, out=None, out_start=0):
        """Every packed row cut at its matches -- the text in front of, between and behind them, empty pieces kept -- as the rows of a NEW
        packed batch -> (out_data, out_offsets, span_offsets) as extract_all_packed.  For patterns that do not match the empty string it
        is re.split / String.split(regex, -1); for nullable patterns it is neither (find-all's enumeration of empty matches differs).
        Device tensors: find_all_packed, split_spans_packed, gather_spans_packed on one stream.  numpy data + offsets:
        needle_gather_matches_packed_host."""
        if isinstance(data, np.ndarray) or not (type(data).__module__.startswith("torch") and data.is_cuda):
            return self._gather_matches_host(_lib.GATHER_PIECES, data, offsets)
        off, st, en = self.find_all_packed(data, offsets, stream=stream)
        po, ps, pe = Pattern.split_spans_packed(data, offsets, off, st, en, stream=stream)
        text, oo = Pattern.gather_spans_packed(data, offsets, po, ps, pe, stream=stream, out=out, out_start=out_start)
        return text, oo, po

    @staticmethod
    def select_rows_packed(data, offsets, bits, stream=None, out=None, out_start=0):
        """The rows a bitmap selects as a NEW packed batch -> (out_data, out_offsets int64[selected + 1]).  bits: the bitmap words of
        contained_in_packed / matches_packed (int64 / uint64, bit r of word r // 64), or a bool tensor of n entries.  The list is built
        with torch -- span_offsets = the prefix sum of the bits, every span (0, 2^31 - 1): the clamp makes it the whole row -- and goes
        through gather_spans_packed.  numpy inputs are uploaded and the result brought back."""
        import torch
        if isinstance(data, np.ndarray):
            b = np.ascontiguousarray(bits)
            b = (b.astype(bool), np.bool_) if b.dtype == np.bool_ else (b.view(np.int64) if b.dtype == np.uint64 else b.astype(np.int64), np.int64)
            d, (o, bt) = Pattern._gather_host_args(data, ((offsets, np.int64), b))
            text, oo = Pattern.select_rows_packed(d, o, bt, stream)
            return Pattern._gather_host_text(text), oo.cpu().numpy()
        n, dv = offsets.numel() - 1, data.device
        one = torch.cuda.current_stream(dv) if stream is None else torch.cuda.ExternalStream(stream, device=dv)
        with torch.cuda.device(dv), torch.cuda.stream(one):
            if bits.dtype == torch.bool:
                assert bits.numel() == n, "bits: one bool per row"
                hit = bits
            else:
                assert bits.numel() >= (n + 63) // 64, "bits: ceil(n / 64) bitmap words"
                hit = ((bits.view(torch.int64).unsqueeze(1) >> torch.arange(64, device=dv)) & 1).reshape(-1)[:n].bool()
            so = torch.zeros(n + 1, dtype=torch.int64, device=dv)
            if n:
                torch.cumsum(hit, 0, out=so[1:])
            chosen = int(so[-1].item())
            st = torch.zeros(chosen, dtype=torch.int32, device=dv)
            en = torch.full((chosen,), 0x7FFFFFFF, dtype=torch.int32, device=dv)
        return Pattern.gather_spans_packed(data, offsets, so, st, en, stream=stream, out=out, out_start=out_start)

    def grep_packed(self, data, offsets, stream=None, out=None, out_start=0):
        """The packed rows that contain a match, as a NEW packed batch -> (out_data, out_offsets): contained_in_packed, then
        select_rows_packed -- what grep prints."""
        if isinstance(data, np.ndarray):
            return Pattern.select_rows_packed(data, offsets, self.contained_in_packed(data, offsets), stream)
        return Pattern.select_rows_packed(data, offsets, self.contained_in_packed(data, offsets, stream=stream), stream=stream, out=out, out_start=out_start)

    @staticmethod
    def _rows_of(text, off, span_off, decode):
        text, off, span_off = np.asarray(text), np.asarray(off), np.asarray(span_off)
        rows = [decode(text[off[m]:off[m + 1]]) for m in range(off.size - 1)]
        return [rows[int(span_off[r]):int(span_off[r + 1])] for r in range(span_off.size - 1)]

    def extract_all_strings(self, strings):
        """Every match of every str, as text -> list of list[str] (re.findall for patterns without groups): pack_strings +
        extract_all_packed."""
        data, offsets = pack_strings(strings)
        text, off, so = self.extract_all_packed(data, offsets)
        return Pattern._rows_of(text, off, so, lambda u: u.tobytes().decode("utf-16-le", "surrogatepass"))

    def split_strings(self, strings):
        """Every str cut at its matches -> list of list[str] (re.split for patterns that do not match the empty string): pack_strings +
        split_packed."""
        data, offsets = pack_strings(strings)
        text, off, so = self.split_packed(data, offsets)
        return Pattern._rows_of(text, off, so, lambda u: u.tobytes().decode("utf-16-le", "surrogatepass"))

    def grep_strings(self, strings):
        """The strs that contain a match -> list[str]: pack_strings + grep_packed."""
        data, offsets = pack_strings(strings)
        text, off = self.grep_packed(data, offsets)
        return [text[off[m]:off[m + 1]].tobytes().decode("utf-16-le", "surrogatepass") for m in range(off.size - 1)]

    def _gather_bytes(self, rows, split):
        data, offsets = pack_bytes(rows)
        d, o, _ = Pattern._utf8_dev(data, offsets)
        moff, bs, be = self.find_all_utf8_packed(d, o)
        if split:
            moff, bs, be = Pattern.split_spans_packed(d, o, moff, bs, be)
        text, off = Pattern.gather_spans_packed(d, o, moff, bs, be)
        return Pattern._rows_of(text.cpu().numpy(), off.cpu().numpy(), moff.cpu().numpy(), lambda u: u.tobytes())

    def extract_all_bytes(self, rows):
        """Every match of every UTF-8 `bytes` row, as bytes -> list of list[bytes]: find_all_utf8_packed's byte positions, then
        gather_spans_packed at char width 1 on the ORIGINAL bytes -- the gather never sees a pattern, and no encoder back to UTF-8 is
        involved."""
        return self._gather_bytes(rows, False)

    def split_bytes(self, rows):
        """Every UTF-8 `bytes` row cut at its matches -> list of list[bytes]; the bytes of ill-formed input outside the matches come back
        untouched (find_all_utf8_packed, split_spans_packed, gather_spans_packed at char width 1)."""
        return self._gather_bytes(rows, True)

    # ---- UTF-8 packed rows: transcoded on the device, byte positions back (needle_utf16_*_from_utf8_packed_dev,
    # needle_utf8_positions_packed_dev, needle_*_utf8_packed_host)
    @staticmethod
    def _utf8_dev(data, offsets):
        """numpy UTF-8 bytes + offsets on the device (padded to whole 4 bytes) -> (data, offsets, True); device tensors as they are."""
        import torch
        if isinstance(data, np.ndarray):
            data = np.ascontiguousarray(data, dtype=np.uint8)
            data = torch.from_numpy(np.concatenate([data, np.zeros(4 + (-data.size) % 4, np.uint8)])).to("cuda")
            return data, torch.from_numpy(np.ascontiguousarray(offsets).astype(np.int64)).to("cuda"), True
        assert data.is_cuda and data.dim() == 1 and data.is_contiguous() and data.dtype == torch.uint8, "data: 1-D uint8 UTF-8 bytes"
        assert isinstance(offsets, torch.Tensor) and offsets.device == data.device and offsets.dtype == torch.int64 and offsets.dim() == 1 \
            and offsets.is_contiguous() and offsets.numel() >= 1, "offsets: 1-D int64, n + 1 entries, on data's device"
        return data, offsets, False

    @staticmethod
    def utf16_from_utf8_packed(data, offsets, stream=None, out=None, out_start=0):
        """UTF-8 packed rows (1-D uint8 bytes, int64 offsets[n + 1]; device tensors) -> (units int16, unit_offsets int64[n + 1],
        non_ascii_words int64, malformed_words int64): the rows as bytes.decode("utf-8", "replace") / new String(bytes, UTF_8) gives them,
        a packed batch of char width 2 for every *_packed method.  needle_utf16_lengths_from_utf8_packed_dev, torch cumsum,
        needle_utf16_from_utf8_packed_dev on one stream, as splice_packed; the one host read is the total.  out / out_start: a
        caller-owned int16 tensor, the result starting at its unit out_start (unit_offsets are positions in it; units outside
        [unit_offsets[0], unit_offsets[n]) are left as they are).  numpy inputs are uploaded and the results brought back."""
        import torch
        L = _lib.lib()
        data, offsets, host = Pattern._utf8_dev(data, offsets)
        n, dv = offsets.numel() - 1, data.device
        v = _lib.PackedView()
        v.data, v.char_width, v.n_rows, v.offsets = data.data_ptr(), 1, n, offsets.data_ptr()
        one = torch.cuda.current_stream(dv) if stream is None else torch.cuda.ExternalStream(stream, device=dv)
        with torch.cuda.device(dv), torch.cuda.stream(one):
            s = one.cuda_stream
            words = (n + 63) // 64
            room = torch.empty(n + 2 * words + 1, dtype=torch.int64, device=dv)  # (never an empty allocation: its pointer, and an empty view's, is NULL)
            lens, na, mal = room[:n], room[n:n + words], room[n + words:n + 2 * words]
            _check(L.needle_utf16_lengths_from_utf8_packed_dev(ctypes.byref(v), room.data_ptr(), room.data_ptr() + 8 * n, room.data_ptr() + 8 * (n + words), s))
            uoff = torch.full((n + 1,), int(out_start), dtype=torch.int64, device=dv)
            if n:
                uoff[1:] += torch.cumsum(lens, 0)
            total = int(uoff[-1].item())
            if out is None:
                text = torch.empty(total + 4, dtype=torch.int16, device=dv)
                out = text[:total]
            else:
                assert out.device == dv and out.dtype == torch.int16 and out.dim() == 1 and out.is_contiguous() and out.numel() >= total
                text = out
            _check(L.needle_utf16_from_utf8_packed_dev(ctypes.byref(v), uoff.data_ptr(), text.data_ptr(), s))
        if host:
            return out.cpu().numpy().view(np.uint16), uoff.cpu().numpy(), na.cpu().numpy().view(np.uint64), mal.cpu().numpy().view(np.uint64)
        return out, uoff, na, mal

    @staticmethod
    def utf8_positions_packed(data, offsets, list_offsets, unit_pos, stream=None, out=None):
        """Code-unit positions of the rows' UTF-16 form -> byte offsets into the UTF-8 rows (needle_utf8_positions_packed_dev): a CSR list
        over the rows (list_offsets int64[n + 1], unit_pos int32) -> byte_pos int32, indexed like unit_pos.  The second unit of a surrogate
        pair maps to the start of its sequence, positions behind the row's end to its length, negative ones to -1.  out: a caller-owned
        int32 tensor (entries outside [list_offsets[0], list_offsets[n]) are left as they are).  numpy inputs are uploaded."""
        import torch
        L = _lib.lib()
        data, offsets, host = Pattern._utf8_dev(data, offsets)
        dv, n = data.device, offsets.numel() - 1
        if host:
            list_offsets = torch.from_numpy(np.ascontiguousarray(list_offsets).astype(np.int64)).to(dv)
            unit_pos = torch.from_numpy(np.ascontiguousarray(unit_pos).astype(np.int32)).to(dv)
        for t, dt, what in ((list_offsets, torch.int64, "list_offsets"), (unit_pos, torch.int32, "unit_pos")):
            assert isinstance(t, torch.Tensor) and t.device == dv and t.dtype == dt and t.dim() == 1 and t.is_contiguous(), what
        assert list_offsets.numel() == n + 1
        if out is None:
            out = torch.empty(unit_pos.numel(), dtype=torch.int32, device=dv)
        else:
            assert out.device == dv and out.dtype == torch.int32 and out.dim() == 1 and out.is_contiguous() and out.numel() >= unit_pos.numel()
        v = _lib.PackedView()
        v.data, v.char_width, v.n_rows, v.offsets = data.data_ptr(), 1, n, offsets.data_ptr()
        with torch.cuda.device(dv):
            s = torch.cuda.current_stream(dv).cuda_stream if stream is None else stream
            some = unit_pos.numel() > 0
            _check(L.needle_utf8_positions_packed_dev(ctypes.byref(v), list_offsets.data_ptr(), unit_pos.data_ptr() if some else None,
                                                      out.data_ptr() if some else None, s))
        return out.cpu().numpy() if host else out

    def _scan_utf8_packed(self, op, data, offsets, stream):
        import torch
        data, offsets, host = Pattern._utf8_dev(data, offsets)
        one = torch.cuda.current_stream(data.device) if stream is None else torch.cuda.ExternalStream(stream, device=data.device)
        with torch.cuda.device(data.device), torch.cuda.stream(one):
            # (the caller's `stream` as it came: None stays None, and both steps then take torch's current stream)
            units, uoff, _, _ = Pattern.utf16_from_utf8_packed(data, offsets, stream=stream)
            words = self._run_packed_dev(op, units, uoff, stream, None)
        return words.cpu().numpy().view(np.uint64) if host else words

    def _utf8_host_view(self, data, offsets):
        data = np.ascontiguousarray(data, dtype=np.uint8)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        v = _lib.PackedView()
        v.data, v.char_width, v.n_rows, v.offsets = data.ctypes.data, 1, offsets.size - 1, offsets.ctypes.data
        return v, (data, offsets)

    def contained_in_utf8_packed(self, data, offsets, stream=None, malformed=False):
        """Bitmap words of containedIn() of every UTF-8 packed row, the pattern seeing the row's decoded text.  Device tensors:
        utf16_from_utf8_packed, then contained_in_packed on the UTF-16 batch, on one stream.  numpy data + offsets:
        needle_contained_in_utf8_packed_host; malformed=True -> (words, malformed_words: the rows that hold ill-formed UTF-8)."""
        if not isinstance(data, np.ndarray):
            assert not malformed, "malformed words: utf16_from_utf8_packed gives them on the device"
            return self._scan_utf8_packed("contained_in", data, offsets, stream)
        L = _lib.lib()
        v, keep = self._utf8_host_view(data, offsets)
        words = np.zeros((v.n_rows + 63) // 64, dtype=np.uint64)
        mal = np.zeros_like(words)
        _check(L.needle_contained_in_utf8_packed_host(self._h, ctypes.byref(v), words.ctypes.data, mal.ctypes.data))
        return (words, mal) if malformed else words

    def matches_utf8_packed(self, data, offsets, stream=None):
        """Bitmap words of matches() of every UTF-8 packed row's decoded text (device chain; numpy inputs are uploaded)."""
        return self._scan_utf8_packed("matches", data, offsets, stream)

    def find_all_utf8_packed(self, data, offsets, stream=None):
        """Every non-overlapping match of every UTF-8 packed row -> (match_offsets int64[n + 1], byte_start int32[m], byte_end int32[m]):
        the matches find_all_packed files on the rows' decoded text, as BYTE offsets into the rows -- what splice_packed takes with the
        original bytes.  Device tensors: utf16_from_utf8_packed, find_all_packed, utf8_positions_packed on start and on end, one
        stream.  numpy data + offsets: needle_find_all_csr_utf8_packed_host."""
        if isinstance(data, np.ndarray):
            L = _lib.lib()
            v, keep = self._utf8_host_view(data, offsets)
            out = np.zeros(v.n_rows + 1, dtype=np.uint64)
            capacity = max(1024, 2 * v.n_rows)
            while True:  # (first with a guessed capacity, then with the exact total)
                st = np.empty(capacity, dtype=np.int32)
                en = np.empty(capacity, dtype=np.int32)
                total = ctypes.c_uint64(0)
                _check(L.needle_find_all_csr_utf8_packed_host(self._h, ctypes.byref(v), out.ctypes.data, st.ctypes.data, en.ctypes.data, capacity,
                                                              ctypes.byref(total), None))
                if total.value <= capacity:
                    return out.astype(np.int64), st[:total.value], en[:total.value]
                capacity = int(total.value)
        import torch
        data, offsets, _ = Pattern._utf8_dev(data, offsets)
        one = torch.cuda.current_stream(data.device) if stream is None else torch.cuda.ExternalStream(stream, device=data.device)
        with torch.cuda.device(data.device), torch.cuda.stream(one):
            s = one.cuda_stream
            units, uoff, _, _ = Pattern.utf16_from_utf8_packed(data, offsets, stream=s)
            moff, st, en = self.find_all_packed(units, uoff, stream=s)
            bs = Pattern.utf8_positions_packed(data, offsets, moff, st, stream=s)
            be = Pattern.utf8_positions_packed(data, offsets, moff, en, stream=s)
        return moff, bs, be

    def find_all_bytes(self, rows):
        """Every non-overlapping match of every UTF-8 `bytes` row -> list of [(byte_start, byte_end), ...] per row: pack_bytes +
        find_all_utf8_packed, the counterpart of find_all_strings for text that is not a str."""
        data, offsets = pack_bytes(rows)
        off, st, en = self.find_all_utf8_packed(data, offsets)
        return [list(zip(st[off[i]:off[i + 1]].tolist(), en[off[i]:off[i + 1]].tolist())) for i in range(len(rows))]

    # ---- capturing groups: the group spans of every span of a match list (needle_pattern_captures_*, needle_captures_spans_packed_dev)
    def captures_info(self, char_width=1):
        """needle_pattern_captures_info as a dict: available, reason (None | "NULLABLE_LOOP" | "NO_REGEX" | "TOO_MANY_GROUPS" | "TOO_BIG"),
        n_groups, and for available programs n_states, n_cols, max_threads, n_slots, n_op_lists, n_ops, start, init_op, lds_bytes.  Needs no
        device."""
        o = _lib.CapturesInfo()
        _check(_lib.lib().needle_pattern_captures_info(self._h, char_width, ctypes.byref(o)))
        d = {k: getattr(o, k) for k, _ in o._fields_}
        d["available"] = bool(o.available)
        d["reason"] = _lib.CAPTURES_REASONS[o.reason]
        return d

    def group_count(self):
        """The pattern's capturing groups, numbered by their opening parenthesis (patterns without regex text raise)."""
        n = self.captures_info()["n_groups"]
        if n < 0:
            raise PatternException("the pattern has no regex text (from_tables / from_bytes): its groups are unknown")
        return n

    def captures_tables(self, char_width=1):
        """needle_pattern_captures_tables as a dict of numpy arrays (class_map uint8[65536], next / op_id int32[n_states, n_cols], op_off,
        ops int32[n_ops, 2] = (dst, src), fin) with captures_info's numbers beside them: the tagged automaton, to be walked on the CPU."""
        info = self.captures_info(char_width)
        cells = info["n_states"] * info["n_cols"]
        t = dict(info, class_map=np.zeros(65536, np.uint8), next=np.zeros(cells, np.int32), op_id=np.zeros(cells, np.int32),
                 op_off=np.zeros(info["n_op_lists"] + 1, np.int32), ops=np.zeros(2 * info["n_ops"], np.int32), fin=np.zeros(info["n_states"], np.int32))
        _check(_lib.lib().needle_pattern_captures_tables(self._h, char_width, t["class_map"].ctypes.data, t["next"].ctypes.data, t["op_id"].ctypes.data, cells,
                                                         t["op_off"].ctypes.data, t["op_off"].size, t["ops"].ctypes.data, t["ops"].size,
                                                         t["fin"].ctypes.data, t["fin"].size))
        t["next"], t["op_id"], t["ops"] = t["next"].reshape(info["n_states"], -1), t["op_id"].reshape(info["n_states"], -1), t["ops"].reshape(-1, 2)
        return t

    def captures_spans_packed(self, data, offsets, span_offsets, start, end, stream=None, out=None):
        """needle_captures_spans_packed_dev: the capturing groups of each span of a CSR span list over packed rows -> (gstart, gend), int32
        device tensors [G + 1, M] indexed like `start` in their second dimension: row g holds group g of a full match of row[start:end]
        (group 0 the clamped span itself), -1 everywhere where the pattern does not match that text whole, (-1, -1) for a group the match
        did not pass.  span_offsets int64[n_rows + 1], start / end int32 -- what find_all_packed returns; spans are clamped into their rows
        and need not be monotone or disjoint; columns below span_offsets[0] are untouched.  out: a caller-owned pair of such tensors
        (second dimension at least M).  Stream-ordered, no host synchronisation.  numpy inputs are uploaded and the planes brought back."""
        import torch
        L = _lib.lib()
        if isinstance(data, np.ndarray):
            d, (o, so, st, en) = Pattern._gather_host_args(data, ((offsets, np.int64), (span_offsets, np.int64), (start, np.int32), (end, np.int32)))
            gs, ge = self.captures_spans_packed(d, o, so, st, en, stream)
            return gs.cpu().numpy(), ge.cpu().numpy()
        Pattern._gather_check(data, ((offsets, torch.int64, "offsets"), (span_offsets, torch.int64, "span_offsets"), (start, torch.int32, "start"),
                                     (end, torch.int32, "end")))
        n, dv, m = offsets.numel() - 1, data.device, start.numel()
        assert n >= 0 and span_offsets.numel() == n + 1 and end.numel() == m, "span_offsets: n_rows + 1 entries; start / end alike"
        planes = self.group_count() + 1
        v = _lib.PackedView()
        v.data, v.char_width, v.n_rows, v.offsets = data.data_ptr(), data.element_size(), n, offsets.data_ptr()
        with torch.cuda.device(dv):
            s = torch.cuda.current_stream(dv).cuda_stream if stream is None else stream
            if out is not None:
                gs, ge = out
                for t in (gs, ge):
                    assert t.device == dv and t.dtype == torch.int32 and t.dim() == 2 and t.is_contiguous() and t.size(0) == planes and t.size(1) >= m
                assert gs.size(1) == ge.size(1)
            else:
                gs = torch.empty((planes, m), dtype=torch.int32, device=dv)
                ge = torch.empty((planes, m), dtype=torch.int32, device=dv)
            some = m > 0
            _check(L.needle_captures_spans_packed_dev(self._h, ctypes.byref(v), span_offsets.data_ptr(), start.data_ptr() if some else None,
                                                      end.data_ptr() if some else None, gs.data_ptr() if some else None,
                                                      ge.data_ptr() if some else None, gs.size(1), s))
        return gs, ge

    def find_all_groups_packed(self, data, offsets, stream=None):
        """Every non-overlapping match of every packed row with its groups -> (match_offsets int64[n_rows + 1], gstart, gend int32[G + 1, m]):
        find_all_packed, then captures_spans_packed on its list, on one stream; row 0 of the planes is the match list itself.  numpy inputs
        are uploaded and the results brought back."""
        if isinstance(data, np.ndarray):
            d, (o,) = Pattern._gather_host_args(data, ((offsets, np.int64),))
            off, gs, ge = self.find_all_groups_packed(d, o, stream)
            return off.cpu().numpy(), gs.cpu().numpy(), ge.cpu().numpy()
        off, st, en = self.find_all_packed(data, offsets, stream)
        gs, ge = self.captures_spans_packed(data, offsets, off, st, en, stream)
        return off, gs, ge

    def extract_group_packed(self, data, offsets, g, stream=None):
        """Group g of every match of every packed row as a NEW packed batch -> (out_data, out_offsets, match_offsets): find_all_groups_packed,
        then gather_spans_packed on plane g.  A group the match did not pass, (-1, -1), clamps to an empty row."""
        host = isinstance(data, np.ndarray)
        if host:
            data, (offsets,) = Pattern._gather_host_args(data, ((offsets, np.int64),))
        off, gs, ge = self.find_all_groups_packed(data, offsets, stream)
        assert 0 <= g < gs.size(0), "group out of range"
        text, toff = Pattern.gather_spans_packed(data, offsets, off, gs[g].contiguous(), ge[g].contiguous(), stream)
        if host:
            return Pattern._gather_host_text(text), toff.cpu().numpy(), off.cpu().numpy()
        return text, toff, off

    def find_all_groups_strings(self, strings):
        """Every match of every str (UTF-16 code units) with its groups -> per string a list of matches, each a list of (start, end) for
        groups 0 .. G, None for a group the match did not pass (re.finditer's m.span(g), pack_strings + find_all_groups_packed)."""
        data, offsets = pack_strings(strings)
        off, gs, ge = self.find_all_groups_packed(data, offsets)
        return Pattern._groups_rows(off, gs, ge, len(strings))

    @staticmethod
    def _groups_rows(off, gs, ge, n):
        span = lambda s, e: None if s < 0 else (s, e)
        return [[[span(int(gs[g, m]), int(ge[g, m])) for g in range(gs.shape[0])] for m in range(int(off[i]), int(off[i + 1]))] for i in range(n)]

    def find_all_groups_utf8_packed(self, data, offsets, stream=None):
        """Every match of every UTF-8 packed row with its groups, as BYTE offsets into the rows -> (match_offsets, gstart, gend int32[G + 1, m]):
        utf16_from_utf8_packed, find_all_groups_packed on the UTF-16 batch, then utf8_positions_packed on every plane (-1 stays -1), one
        stream.  numpy inputs are uploaded and the results brought back."""
        import torch
        data, offsets, host = Pattern._utf8_dev(data, offsets)
        one = torch.cuda.current_stream(data.device) if stream is None else torch.cuda.ExternalStream(stream, device=data.device)
        with torch.cuda.device(data.device), torch.cuda.stream(one):
            s = one.cuda_stream
            units, uoff, _, _ = Pattern.utf16_from_utf8_packed(data, offsets, stream=s)
            moff, gs, ge = self.find_all_groups_packed(units, uoff, stream=s)
            bs, be = torch.empty_like(gs), torch.empty_like(ge)
            for g in range(gs.size(0)):
                Pattern.utf8_positions_packed(data, offsets, moff, gs[g], stream=s, out=bs[g])
                Pattern.utf8_positions_packed(data, offsets, moff, ge[g], stream=s, out=be[g])
        if host:
            return moff.cpu().numpy(), bs.cpu().numpy(), be.cpu().numpy()
        return moff, bs, be

    def find_all_groups_bytes(self, rows):
        """find_all_groups_strings for UTF-8 `bytes` rows: byte offsets (pack_bytes + find_all_groups_utf8_packed)."""
        data, offsets = pack_bytes(rows)
        off, gs, ge = self.find_all_groups_utf8_packed(data, offsets)
        return Pattern._groups_rows(off, gs, ge, len(rows))

    def replace_all_bytes(self, rows, repl):
        """Every match of every UTF-8 `bytes` row replaced by the bytes `repl` -> list[bytes]: find_all_utf8_packed on the device, then
        splice_packed at char width 1 on the ORIGINAL bytes with the replacement's bytes -- no encoder back to UTF-8 is involved, and the
        bytes of ill-formed input outside the matches come back untouched."""
        data, offsets = pack_bytes(rows)
        d, o, _ = Pattern._utf8_dev(data, offsets)
        moff, bs, be = self.find_all_utf8_packed(d, o)
        text, off = Pattern.splice_packed(d, o, moff, bs, be, np.frombuffer(bytes(repl), dtype=np.uint8))
        text, off = text.cpu().numpy(), off.cpu().numpy()
        return [text[off[i]:off[i + 1]].tobytes() for i in range(len(rows))]

    # ---- replace matches by a template with group references: "$2-$1" (needle_template_parse, needle_replace_groups_*_packed_dev)
    def parse_template(self, repl):
        """A replacement template (a str, read as UTF-16 code units) by the rules of java.util.regex's Matcher.appendReplacement for this
        pattern's group_count() -> (groups, literals): K group numbers and K + 1 literal strs, the template being
        literals[0] + $groups[0] + literals[1] + ... + literals[K].  `\\x` is x, `$12` takes digits while the number names a group, `${name}`
        is refused.  Needs no device; ValueError carries the library's message (position and rule)."""
        L = _lib.lib()
        u = np.ascontiguousarray(_utf16(repl))
        groups = np.zeros(_lib.TEMPLATE_MAX_REFS, dtype=np.int32)
        loff = np.zeros(_lib.TEMPLATE_MAX_REFS + 2, dtype=np.uint32)
        lits = np.zeros(max(u.size, 1), dtype=np.uint16)  # (the literals are never longer than the template)
        k, nl = ctypes.c_uint32(0), ctypes.c_uint32(0)
        rc = L.needle_template_parse(u.ctypes.data if u.size else None, u.size, self.group_count(), groups.ctypes.data, groups.size, loff.ctypes.data,
                                     loff.size, lits.ctypes.data, lits.size, ctypes.byref(k), ctypes.byref(nl))
        if rc == _lib.ERR_INVALID:
            raise ValueError(_lib.last_error())
        _check(rc)
        text = lambda a: a.tobytes().decode("utf-16-le", "surrogatepass")
        return groups[:k.value].tolist(), [text(lits[loff[i]:loff[i + 1]]) for i in range(k.value + 1)]

    @staticmethod
    def _template(groups, literals, char_width, n_planes):
        """(groups, literals) as a needle_template of the rows' char width -> (the structure, the arrays it points into).  ValueError: not
        K + 1 literals, more than 16 references, a group that is no plane, a unit the rows cannot hold, more than 4096 units in all."""
        groups, literals = [int(g) for g in groups], list(literals)
        if len(literals) != len(groups) + 1:
            raise ValueError("a template of K references has K + 1 literals (got %d and %d)" % (len(groups), len(literals)))
        if len(groups) > _lib.TEMPLATE_MAX_REFS:
            raise ValueError("a template holds at most %d group references" % _lib.TEMPLATE_MAX_REFS)
        for g in groups:
            if not 0 <= g < n_planes:
                raise ValueError("group %d is outside the %d planes" % (g, n_planes))
        parts = [Pattern._repl_units(x, char_width) for x in literals]
        loff = np.zeros(len(parts) + 1, dtype=np.uint32)
        loff[1:] = np.cumsum([p.size for p in parts])
        if int(loff[-1]) > _lib.REPLACE_MAX_UNITS:
            raise ValueError("template literals longer than %d code units" % _lib.REPLACE_MAX_UNITS)
        g, units = np.asarray(groups, dtype=np.int32), np.ascontiguousarray(np.concatenate(parts))
        t = _lib.Template()
        t.n_refs, t.groups, t.lit_offsets, t.lits = len(groups), g.ctypes.data if g.size else None, loff.ctypes.data, units.ctypes.data if units.size else None
        return t, (g, loff, units)

    @staticmethod
    def splice_groups_packed(data, offsets, match_offsets, gstart, gend, groups, literals, stream=None, out=None, out_start=0):
        """splice_packed with a TEMPLATE per match (needle_replace_groups_lengths_packed_dev, torch cumsum,
        needle_replace_groups_fill_packed_dev on one stream): match m of the caller's CSR list -- column m of the int32 planes gstart / gend
        [n_planes, stride], what captures_spans_packed returns, plane 0 the match itself -- is replaced by
        literals[0] + group groups[0] + literals[1] + ... + literals[K], or KEPT where gstart[0, m] < 0; a group with gstart[g, m] < 0
        contributes nothing -> (out_data, out_offsets int64[n + 1]).  groups / literals: what parse_template returns (literals: str or 1-D
        arrays of code units).  Pure: no pattern.  out / out_start (device inputs only) and the one host read: as splice_packed; numpy
        inputs are uploaded, spliced on the device and brought back, and take neither out nor out_start."""
        import torch
        L = _lib.lib()
        if isinstance(data, np.ndarray):
            assert out is None and out_start == 0, "out / out_start go with device inputs"
            d, (o, mo) = Pattern._gather_host_args(data, ((offsets, np.int64), (match_offsets, np.int64)))
            pl = lambda x: torch.from_numpy(np.ascontiguousarray(x, dtype=np.int32)).to("cuda")
            text, off = Pattern.splice_groups_packed(d, o, mo, pl(gstart), pl(gend), groups, literals, stream)
            return Pattern._gather_host_text(text), off.cpu().numpy()
        Pattern._gather_check(data, ((offsets, torch.int64, "offsets"), (match_offsets, torch.int64, "match_offsets")))
        for t, what in ((gstart, "gstart"), (gend, "gend")):
            assert isinstance(t, torch.Tensor) and t.device == data.device and t.dtype == torch.int32 and t.dim() == 2 and t.is_contiguous(), what
        assert gstart.shape == gend.shape, "gstart / gend: two planes arrays of one shape"
        n, dv, cw = offsets.numel() - 1, data.device, data.element_size()
        assert n >= 0 and match_offsets.numel() == n + 1
        planes, stride = gstart.size(0), gstart.size(1)
        tm, keep = Pattern._template(groups, literals, cw, planes)
        v = _lib.PackedView()
        v.data, v.char_width, v.n_rows, v.offsets = data.data_ptr(), cw, n, offsets.data_ptr()
        one = torch.cuda.current_stream(dv) if stream is None else torch.cuda.ExternalStream(stream, device=dv)
        with torch.cuda.device(dv), torch.cuda.stream(one):
            s = one.cuda_stream
            sp, ep = (gstart.data_ptr(), gend.data_ptr()) if gstart.numel() else (None, None)
            lens = torch.empty(n, dtype=torch.int64, device=dv)
            _check(L.needle_replace_groups_lengths_packed_dev(ctypes.byref(v), match_offsets.data_ptr(), sp, ep, stride, planes, ctypes.byref(tm),
                                                              lens.data_ptr(), s))
            out_off = torch.full((n + 1,), int(out_start), dtype=torch.int64, device=dv)
            if n:
                out_off[1:] += torch.cumsum(lens, 0)
            total = int(out_off[-1].item())
            if out is None:
                room = torch.empty(total + 4, dtype=data.dtype, device=dv)  # (never an empty allocation: its pointer would be NULL)
                out = room[:total]
            else:
                assert out.device == dv and out.dtype == data.dtype and out.dim() == 1 and out.is_contiguous() and out.numel() >= total
                room = out
            _check(L.needle_replace_groups_fill_packed_dev(ctypes.byref(v), match_offsets.data_ptr(), sp, ep, stride, planes, ctypes.byref(tm),
                                                           out_off.data_ptr(), room.data_ptr(), s))
        del keep
        return out, out_off

    def _need_captures(self, char_width):
        info = self.captures_info(char_width)
        if not info["available"]:
            raise PatternException("group references need this pattern's capturing groups, which are refused: %s" % info["reason"])

    def replace_all_groups_packed(self, data, offsets, repl, stream=None, out=None, out_start=0):
        """Every match of every packed row -- find_all_packed's list -- replaced by the template `repl` with its group references filled
        in ("$2-$1"; parse_template's syntax) -> (out_data, out_offsets): find_all_groups_packed, then splice_groups_packed, on one
        stream.  java.util.regex's replaceAll(String) wherever the list is its find() loop's (see replace_all_packed).  A pattern whose
        captures are refused raises PatternException with the reason.  numpy inputs are uploaded and the result brought back."""
        groups, literals = self.parse_template(repl)
        host = isinstance(data, np.ndarray)
        self._need_captures(data.itemsize if host else data.element_size())
        if host:
            data, (offsets,) = Pattern._gather_host_args(data, ((offsets, np.int64),))
        off, gs, ge = self.find_all_groups_packed(data, offsets, stream)
        text, toff = Pattern.splice_groups_packed(data, offsets, off, gs, ge, groups, literals, stream=stream, out=out, out_start=out_start)
        return (Pattern._gather_host_text(text), toff.cpu().numpy()) if host else (text, toff)

    def replace_first_groups_packed(self, data, offsets, repl, stream=None, out=None, out_start=0):
        """The first match of every packed row (find_packed's) replaced by the template `repl`: find_packed's results as a list of at most
        one match per row (as replace_first_packed builds it), captures_spans_packed on that list, then splice_groups_packed."""
        import torch
        groups, literals = self.parse_template(repl)
        host = isinstance(data, np.ndarray)
        self._need_captures(data.itemsize if host else data.element_size())
        if host:
            data, (offsets,) = Pattern._gather_host_args(data, ((offsets, np.int64),))
        dv, n = data.device, offsets.numel() - 1
        one = torch.cuda.current_stream(dv) if stream is None else torch.cuda.ExternalStream(stream, device=dv)
        with torch.cuda.device(dv), torch.cuda.stream(one):
            words, st, en = self.find_packed(data, offsets, stream=stream)
            hit = ((words.unsqueeze(1) >> torch.arange(64, device=dv)) & 1).reshape(-1)[:n].bool()
            moff = torch.zeros(n + 1, dtype=torch.int64, device=dv)
            if n:
                torch.cumsum(hit, 0, out=moff[1:])
            st1, en1 = st[:n][hit].contiguous(), en[:n][hit].contiguous()
        gs, ge = self.captures_spans_packed(data, offsets, moff, st1, en1, stream)
        text, toff = Pattern.splice_groups_packed(data, offsets, moff, gs, ge, groups, literals, stream=stream, out=out, out_start=out_start)
        return (Pattern._gather_host_text(text), toff.cpu().numpy()) if host else (text, toff)

    def replace_all_groups_strings(self, strings, repl):
        """Every match of every str replaced by the template `repl` -> list[str] (UTF-16 code units, like java.lang.String):
        pack_strings + replace_all_groups_packed.  compile(r"([0-9]+)-([0-9]+)").replace_all_groups_strings(["10-20"], "$2-$1") == ["20-10"]."""
        data, offsets = pack_strings(strings)
        text, off = self.replace_all_groups_packed(data, offsets, repl)
        return [text[off[i]:off[i + 1]].tobytes().decode("utf-16-le", "surrogatepass") for i in range(len(strings))]

    def replace_all_groups_bytes(self, rows, repl):
        """replace_all_groups_strings for UTF-8 `bytes` rows -> list[bytes]: find_all_groups_utf8_packed for the groups' BYTE positions, then
        splice_groups_packed at char width 1 on the ORIGINAL bytes with each literal of the template (a str) encoded to UTF-8.  No encoder
        runs over the text: the bytes of ill-formed input outside the matches come back untouched."""
        groups, literals = self.parse_template(repl.decode("utf-8") if isinstance(repl, (bytes, bytearray)) else repl)
        self._need_captures(2)
        lits = [np.frombuffer(x.encode("utf-8"), dtype=np.uint8) for x in literals]
        data, offsets = pack_bytes(rows)
        d, o, _ = Pattern._utf8_dev(data, offsets)
        moff, bs, be = self.find_all_groups_utf8_packed(d, o)
        text, off = Pattern.splice_groups_packed(d, o, moff, bs, be, groups, lits)
        text, off = text.cpu().numpy(), off.cpu().numpy()
        return [text[off[i]:off[i + 1]].tobytes() for i in range(len(rows))]

    # ---- a file as a packed batch: lines_packed in front of the UTF-8 chain (needle_lines_*_packed_dev)
    def _grep_lines(self, buf):
        """A UTF-8 file -> (its lines without terminators as a packed device batch, the bitmap words of the lines that contain a match):
        upload, lines_packed, contained_in_utf8_packed on the current stream; None for a file without lines."""
        import torch
        a = np.frombuffer(bytes(buf), dtype=np.uint8)
        if a.size == 0:
            return None
        d = torch.from_numpy(np.concatenate([a, np.zeros(4 + (-a.size) % 4, np.uint8)])).to("cuda")
        text, lo, _ = lines_packed(d[:a.size])
        return (text, lo, self.contained_in_utf8_packed(text, lo)) if lo.numel() > 1 else None

    def grep_lines_bytes(self, buf):
        """The lines of the UTF-8 file `buf` (bytes) that contain a match, without their terminators -> list[bytes]: what
        [l for l in buf.splitlines() if re.search(regex, l.decode("utf-8", "replace"))] gives.  The file is uploaded whole and cut into
        lines on the device (lines_packed); the lines go through contained_in_utf8_packed and select_rows_packed as the byte rows they
        are; one download of the chosen lines.  The host never sees a row before that."""
        r = self._grep_lines(buf)
        if r is None:
            return []
        text, off = Pattern.select_rows_packed(r[0], r[1], r[2])
        text, off = text.cpu().numpy(), off.cpu().numpy()
        return [text[off[i]:off[i + 1]].tobytes() for i in range(off.size - 1)]

    def count_lines_bytes(self, buf):
        """The number of lines of the UTF-8 file `buf` that contain a match (grep -c): grep_lines_bytes without the gather."""
        r = self._grep_lines(buf)
        return 0 if r is None else int(unpack_bitmap(r[2], r[1].numel() - 1).sum())

    @staticmethod
    def rows_from_packed(data, offsets, row_stride=None, stream=None):
        """Device tensors: packed code units (1-D uint8 | int16) + int64 offsets[n + 1] -> (rows [n, row_stride],
        lengths int32[n]) in the fixed-stride layout the scan kernels read.  row_stride defaults to the longest row
        rounded up to 16 bytes (one device->host sync to learn it)."""
        import torch
        L = _lib.lib()
        assert data.is_cuda and data.dim() == 1 and data.is_contiguous() and data.dtype in (torch.uint8, torch.int16, torch.uint16)
        assert offsets.is_cuda and offsets.dtype == torch.int64 and offsets.dim() == 1 and offsets.is_contiguous()
        n = offsets.numel() - 1
        cw = data.element_size()
        per = 16 // cw
        if row_stride is None:
            longest = int((offsets[1:] - offsets[:-1]).max().item()) if n else 0
            row_stride = max(per, (longest + per - 1) // per * per)
        assert row_stride % per == 0
        with torch.cuda.device(data.device):
            s = torch.cuda.current_stream(data.device).cuda_stream if stream is None else stream
            rows = torch.empty((n, row_stride), dtype=data.dtype, device=data.device)
            lengths = torch.empty(n, dtype=torch.int32, device=data.device)
            overflow = torch.zeros(1, dtype=torch.int32, device=data.device)
            v = _lib.PackedView()
            v.data, v.char_width, v.n_rows, v.offsets = data.data_ptr(), cw, n, offsets.data_ptr()
            _check(L.needle_rows_from_packed_dev(ctypes.byref(v), rows.data_ptr(), row_stride, lengths.data_ptr(),
                                                 overflow.data_ptr(), s))
        return rows, lengths, overflow


SET_OPS = {"matches": 0, "contained_in": 1}


class PatternSet:
    """1 .. 32 compiled patterns answered in ONE pass over a packed batch (needle_pattern_set, include/needle_hip.h): bit i of a row's
    mask is what matches() / containedIn() of patterns[i] returns for that row.  The patterns' tables are copied: the Pattern objects
    may go away.  A pattern whose automaton does not fit the LDS as a plain table (a big dictionary) is refused
    (PatternClassCompilationException naming its index)."""

    def __init__(self, patterns):
        patterns = list(patterns)
        arr = (ctypes.c_void_p * max(1, len(patterns)))(*[getattr(p, "_h", None) for p in patterns])
        h = ctypes.c_void_p()
        _check(_lib.lib().needle_pattern_set_create(arr, len(patterns), ctypes.byref(h)))
        self._h = h
        self.n_patterns = len(patterns)
        self.members = [(p.regex, p.flags) for p in patterns]  # (regex source or None, flags) per member: union_pattern()

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h and _lib is not None and _lib._lib is not None:
            _lib._lib.needle_pattern_set_destroy(h)

    def union_pattern(self):
        """The pattern (r0)|(r1)|.. of the members' regex sources in member order, compiled with their common flags: its find-all is
        the span list that tag_matches_packed tags.  ValueError when a member has no regex source (from_tables, from_bytes) or the
        members' flags differ."""
        if any(r is None for r, _ in self.members):
            raise ValueError("union_pattern: member %d has no regex source" % [r is None for r, _ in self.members].index(True))
        flags = {f for _, f in self.members}
        if len(flags) != 1:
            raise ValueError("union_pattern: the members' flags differ")
        return DFACompiler.compile("|".join("(" + r + ")" for r, _ in self.members), flags=flags.pop())

    @staticmethod
    def first_member(masks):
        """Index of the lowest set bit of every mask, -1 for 0 (numpy or torch in, int32 numpy out).  For a union compiled in member
        order (union_pattern) the lowest bit is the convention for "the rule" of a match: the first alternative that matches the span
        whole, as an ordered rule list reads."""
        m = masks.cpu().numpy() if not isinstance(masks, np.ndarray) and type(masks).__module__.startswith("torch") else np.asarray(masks)
        m = np.ascontiguousarray(m).astype(np.int64) & 0xFFFFFFFF
        low = m & -m
        idx = np.zeros(m.shape, dtype=np.int32)
        for b in (16, 8, 4, 2, 1):  # log2 of a power of two
            hit = (low >> b) != 0
            idx += np.where(hit, b, 0).astype(np.int32)
            low = np.where(hit, low >> b, low)
        return np.where(m == 0, -1, idx).astype(np.int32)

    def matches_spans_packed(self, data, offsets, span_offsets, start, end, stream=None, out=None):
        """needle_set_matches_spans_packed_dev (device tensors): which members match each span of a CSR span list over packed rows ->
        an int32 device tensor of masks indexed like `start` (bit i: matches() of patterns[i] on row[start:end]); entries below
        span_offsets[0] are untouched.  span_offsets int64[n_rows + 1], start / end int32 -- what Pattern.find_all_packed returns;
        spans are clamped into their rows and need not be monotone or disjoint.  Stream-ordered, no host synchronisation."""
        import torch
        L = _lib.lib()
        assert data.is_cuda and data.dim() == 1 and data.is_contiguous() and data.dtype in (torch.uint8, torch.int16, torch.uint16), \
            "data: 1-D uint8 or (u)int16 code units on the device"
        for name, t, dt in (("offsets", offsets, torch.int64), ("span_offsets", span_offsets, torch.int64), ("start", start, torch.int32),
                            ("end", end, torch.int32)):
            assert isinstance(t, torch.Tensor) and t.device == data.device and t.dtype == dt and t.dim() == 1 and t.is_contiguous(), \
                "%s: 1-D %s on data's device" % (name, dt)
        n = offsets.numel() - 1
        assert n >= 0 and span_offsets.numel() == n + 1 and start.numel() == end.numel(), "span_offsets: n_rows + 1 entries; start / end alike"
        v = _lib.PackedView()
        v.data, v.char_width, v.n_rows, v.offsets = data.data_ptr(), data.element_size(), n, offsets.data_ptr()
        with torch.cuda.device(data.device):
            s = torch.cuda.current_stream(data.device).cuda_stream if stream is None else stream
            if out is not None:  # a caller-owned result buffer (indexed like start)
                assert out.is_cuda and out.dtype == torch.int32 and out.is_contiguous() and out.numel() >= start.numel()
                masks = out
            else:
                masks = torch.empty(start.numel(), dtype=torch.int32, device=data.device)
            if start.numel() == 0:  # no span, nothing to write (and an empty tensor has no address to hand over)
                return masks
            _check(L.needle_set_matches_spans_packed_dev(self._h, ctypes.byref(v), span_offsets.data_ptr(), start.data_ptr(), end.data_ptr(),
                                                         masks.data_ptr(), s))
        return masks

    def tag_matches_packed(self, pattern, data, offsets, stream=None):
        """Every match of `pattern` in every packed row with the members that match it -> (match_offsets int64[n_rows + 1], start
        int32[m], end int32[m], masks[m]).  Device tensors: pattern.find_all_packed, then matches_spans_packed on the same stream
        (stream-ordered apart from the total that find_all_packed reads back); masks int32.  numpy data + offsets:
        needle_set_tag_matches_packed_host; masks uint32."""
        L = _lib.lib()
        if isinstance(data, np.ndarray) or not (type(data).__module__.startswith("torch") and data.is_cuda):
            data = np.ascontiguousarray(data)
            if data.dtype == np.int16:
                data = data.view(np.uint16)
            assert data.ndim == 1 and data.dtype in (np.uint8, np.uint16), "data: 1-D uint8/uint16 code units"
            offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
            n = offsets.size - 1
            v = _lib.PackedView()
            v.data, v.char_width, v.n_rows, v.offsets = data.ctypes.data, data.dtype.itemsize, n, offsets.ctypes.data
            out = np.zeros(n + 1, dtype=np.uint64)
            capacity = max(1024, 2 * n)
            while True:  # (first with a guessed capacity, then with the exact total)
                st = np.empty(capacity, dtype=np.int32)
                en = np.empty(capacity, dtype=np.int32)
                masks = np.zeros(capacity, dtype=np.uint32)
                total = ctypes.c_uint64(0)
                _check(L.needle_set_tag_matches_packed_host(self._h, pattern._h, ctypes.byref(v), out.ctypes.data, st.ctypes.data, en.ctypes.data,
                                                            masks.ctypes.data, capacity, ctypes.byref(total)))
                if total.value <= capacity:
                    return out.astype(np.int64), st[:total.value], en[:total.value], masks[:total.value]
                capacity = int(total.value)
        off, st, en = pattern.find_all_packed(data, offsets, stream)
        return off, st, en, self.matches_spans_packed(data, offsets, off, st, en, stream)

    def find_all_tagged_strings(self, pattern, strings):
        """Every match of `pattern` in every str (UTF-16 code units) with its member mask -> per string a list of (start, end, mask)
        (pack_strings + the host entry)."""
        data, offsets = pack_strings(strings)
        off, st, en, masks = self.tag_matches_packed(pattern, data, offsets)
        return [list(zip(st[off[i]:off[i + 1]].tolist(), en[off[i]:off[i + 1]].tolist(), masks[off[i]:off[i + 1]].tolist()))
                for i in range(len(strings))]

    # ---- a rule list: rule i -> replacement i (needle_replace_each_*_packed_dev / needle_set_replace_each_packed_host)
    def replace_each_packed(self, pattern, data, offsets, repls, stream=None, out=None, out_start=0):
        """Every match of `pattern` in every packed row replaced by repls[i], i the LOWEST member of the set that matches the span whole
        (first_member's convention: the first rule of an ordered rule list); a match no member matches is kept as it is ->
        (out_data, out_offsets[n + 1]).  repls: one str or 1-D array of code units per member.  Device tensors: tag_matches_packed, then
        Pattern.splice_each_packed(lowest_bit=True) on the same stream -- the masks go in as they are.  out / out_start: as
        Pattern.splice_packed.  numpy data + offsets: needle_set_replace_each_packed_host."""
        L = _lib.lib()
        repls = list(repls)
        if len(repls) != self.n_patterns:
            raise ValueError("one replacement per member of the set: %d members, %d replacements" % (self.n_patterns, len(repls)))
        if isinstance(data, np.ndarray) or not (type(data).__module__.startswith("torch") and data.is_cuda):
            data = np.ascontiguousarray(data)
            if data.dtype == np.int16:
                data = data.view(np.uint16)
            assert data.ndim == 1 and data.dtype in (np.uint8, np.uint16), "data: 1-D uint8/uint16 code units"
            offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
            n = offsets.size - 1
            r, roff = Pattern._repl_table(repls, data.dtype.itemsize)
            v = _lib.PackedView()
            v.data, v.char_width, v.n_rows, v.offsets = data.ctypes.data, data.dtype.itemsize, n, offsets.ctypes.data
            out_off = np.zeros(n + 1, dtype=np.uint64)
            capacity = max(1024, 2 * int(offsets[-1] - offsets[0]))
            while True:  # (first with a guessed capacity, then with the exact total)
                text = np.empty(capacity, dtype=data.dtype)
                total = ctypes.c_uint64(0)
                _check(L.needle_set_replace_each_packed_host(self._h, pattern._h, ctypes.byref(v), r.ctypes.data if r.size else None, roff.ctypes.data,
                                                             roff.size - 1, out_off.ctypes.data, text.ctypes.data, capacity, ctypes.byref(total)))
                if total.value <= capacity:
                    return text[:total.value], out_off.astype(np.int64)
                capacity = int(total.value)
        off, st, en, masks = self.tag_matches_packed(pattern, data, offsets, stream)
        return Pattern.splice_each_packed(data, offsets, off, st, en, masks, repls, stream=stream, out=out, out_start=out_start, lowest_bit=True)

    def replace_each_strings(self, strings, repls, pattern=None):
        """Every match of `pattern` (default: union_pattern()) in every str replaced by its rule's str of `repls` -> list[str] (UTF-16
        code units, like java.lang.String): pack_strings + replace_each_packed's host entry."""
        pattern = self.union_pattern() if pattern is None else pattern
        data, offsets = pack_strings(strings)
        text, off = self.replace_each_packed(pattern, data, offsets, repls)
        return [text[off[i]:off[i + 1]].tobytes().decode("utf-16-le", "surrogatepass") for i in range(len(strings))]

    def replace_each_bytes(self, rows, repls, pattern=None):
        """Every match of `pattern` (default: union_pattern()) in every UTF-8 `bytes` row replaced by its rule's `bytes` of `repls` ->
        list[bytes].  The composition of Pattern.replace_all_bytes: utf16_from_utf8_packed, find_all_packed and matches_spans_packed on the
        UTF-16 view, utf8_positions_packed on start and end, then splice_each_packed at char width 1 on the ORIGINAL bytes -- no encoder
        back to UTF-8, and ill-formed bytes outside replaced matches come back untouched."""
        pattern = self.union_pattern() if pattern is None else pattern
        repls = [np.frombuffer(bytes(r), dtype=np.uint8) for r in repls]
        if len(repls) != self.n_patterns:
            raise ValueError("one replacement per member of the set: %d members, %d replacements" % (self.n_patterns, len(repls)))
        data, offsets = pack_bytes(rows)
        d, o, _ = Pattern._utf8_dev(data, offsets)
        units, uoff, _, _ = Pattern.utf16_from_utf8_packed(d, o)
        moff, st, en = pattern.find_all_packed(units, uoff)
        masks = self.matches_spans_packed(units, uoff, moff, st, en)
        bs = Pattern.utf8_positions_packed(d, o, moff, st)
        be = Pattern.utf8_positions_packed(d, o, moff, en)
        text, off = Pattern.splice_each_packed(d, o, moff, bs, be, masks, repls, lowest_bit=True)
        text, off = text.cpu().numpy(), off.cpu().numpy()
        return [text[off[i]:off[i + 1]].tobytes() for i in range(len(rows))]

    def info(self, op="contained_in", char_width=1):
        """The groups of one op and char width (host-side: needs no GPU): {"n_patterns", "n_groups", "groups": [{"first_pattern",
        "pattern_count", "n_states", "n_columns", "kernel_mode", "lds_bytes"}, ...]}."""
        i = _lib.SetInfo()
        _check(_lib.lib().needle_pattern_set_info(self._h, SET_OPS[op], int(char_width), ctypes.byref(i)))
        keys = ("first_pattern", "pattern_count", "n_states", "n_columns", "kernel_mode", "lds_bytes")
        return {"n_patterns": i.n_patterns, "n_groups": i.n_groups,
                "groups": [{k: getattr(i, k)[g] for k in keys} for g in range(i.n_groups)]}

    def tables(self, op="contained_in", char_width=1, group=0):
        """One group's product automaton on the host: {"class_map" uint8[65536], "n_classes", "n_states", "start", "table" int32[n_states,
        n_classes] (-1: every component dead), "masks" uint32[n_states]}."""
        L = _lib.lib()
        nc, ns, st = ctypes.c_int32(0), ctypes.c_int32(0), ctypes.c_int32(0)
        args = (self._h, SET_OPS[op], int(char_width), int(group))
        _check(L.needle_pattern_set_get_tables(*args, None, ctypes.byref(nc), ctypes.byref(ns), ctypes.byref(st), None, 0, None, 0))
        cm = np.zeros(65536, dtype=np.uint8)
        table = np.zeros(ns.value * nc.value, dtype=np.int32)
        masks = np.zeros(ns.value, dtype=np.uint32)
        _check(L.needle_pattern_set_get_tables(*args, cm.ctypes.data, None, None, None, table.ctypes.data, table.size, masks.ctypes.data, masks.size))
        return {"class_map": cm, "n_classes": nc.value, "n_states": ns.value, "start": st.value,
                "table": table.reshape(ns.value, nc.value), "masks": masks}

    def _run_packed(self, op, data, offsets, stream, out):
        L = _lib.lib()
        if not isinstance(data, np.ndarray) and type(data).__module__.startswith("torch") and data.is_cuda:
            import torch
            assert data.dim() == 1 and data.is_contiguous() and data.dtype in (torch.uint8, torch.int16, torch.uint16), \
                "data: 1-D uint8 or (u)int16 code units"
            assert isinstance(offsets, torch.Tensor) and offsets.is_cuda and offsets.device == data.device, "offsets: on data's device"
            assert offsets.dtype == torch.int64 and offsets.dim() == 1 and offsets.is_contiguous() and offsets.numel() >= 1, \
                "offsets: 1-D int64, n + 1 entries"
            n = offsets.numel() - 1
            v = _lib.PackedView()
            v.data, v.char_width, v.n_rows, v.offsets = data.data_ptr(), data.element_size(), n, offsets.data_ptr()
            with torch.cuda.device(data.device):
                s = torch.cuda.current_stream(data.device).cuda_stream if stream is None else stream
                if out is not None:  # a caller-owned result buffer (at least n_rows int32)
                    assert out.is_cuda and out.dtype == torch.int32 and out.is_contiguous() and out.numel() >= n
                    masks = out
                else:
                    masks = torch.empty(n, dtype=torch.int32, device=data.device)
                fn = L.needle_set_matches_packed_dev if op == "matches" else L.needle_set_contained_in_packed_dev
                _check(fn(self._h, ctypes.byref(v), masks.data_ptr(), s))
            return masks
        data = np.ascontiguousarray(data)
        if data.dtype == np.int16:
            data = data.view(np.uint16)
        assert data.ndim == 1 and data.dtype in (np.uint8, np.uint16), "data: 1-D uint8/uint16 code units"
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        n = offsets.size - 1
        v = _lib.PackedView()
        v.data, v.char_width, v.n_rows, v.offsets = data.ctypes.data, data.dtype.itemsize, n, offsets.ctypes.data
        masks = np.zeros(n, dtype=np.uint32)
        fn = L.needle_set_matches_packed_host if op == "matches" else L.needle_set_contained_in_packed_host
        _check(fn(self._h, ctypes.byref(v), masks.ctypes.data))
        return masks

    def matches_packed(self, data, offsets, stream=None, out=None):
        """Masks of matches() of every packed row.  Device tensors (1-D uint8 | (u)int16 data, int64 offsets[n + 1]) ->
        needle_set_matches_packed_dev, an int32 device tensor of n_rows masks (bit i: patterns[i]; stream-ordered); numpy data + offsets
        -> needle_set_matches_packed_host, uint32[n_rows]."""
        return self._run_packed("matches", data, offsets, stream, out)

    def contained_in_packed(self, data, offsets, stream=None, out=None):
        """Masks of containedIn() of every packed row (as matches_packed)."""
        return self._run_packed("contained_in", data, offsets, stream, out)

    def matches_strings(self, strings):
        """matches() masks of a list of str (UTF-16 code units, like java.lang.String): pack_strings + the host entry -> uint32[n]."""
        return self.matches_packed(*pack_strings(strings))

    def contained_in_strings(self, strings):
        """containedIn() masks of a list of str -> uint32[n]."""
        return self.contained_in_packed(*pack_strings(strings))


def pack_strings(strings):
    """list[str] -> (uint16 code units back to back, uint64 offsets[n + 1])."""
    units = [_utf16(x) for x in strings]
    offsets = np.zeros(len(units) + 1, dtype=np.uint64)
    if units:
        offsets[1:] = np.cumsum([u.size for u in units])
    data = np.concatenate(units) if units else np.zeros(0, dtype=np.uint16)
    return data.astype(np.uint16), offsets


def pack_bytes(rows):
    """list[bytes] (UTF-8, or whatever the rows hold) -> (uint8 bytes back to back, uint64 offsets[n + 1]): the layout of an Arrow string column."""
    offsets = np.zeros(len(rows) + 1, dtype=np.uint64)
    if rows:
        offsets[1:] = np.cumsum([len(x) for x in rows])
    return np.frombuffer(b"".join(bytes(x) for x in rows), dtype=np.uint8).copy(), offsets


def lines_packed(data, offsets=None, keep_ends=False, stream=None, out=None, out_start=0, line_start=0):
    """A packed batch of DOCUMENTS (text buffers: files, multi-line cells) cut at its line terminators into a packed batch of LINES, on the
    device -> (text, line_offsets, doc_line_offsets): bytes.splitlines() / String.lines() of every document, one after the other.
    data: 1-D uint8 or int16 / uint16 code units; offsets: int64[n + 1], None = one document, the whole tensor.  '\\n', '\\r' and '\\r\\n' end a
    line (whole code units: U+2028, U+0085 and 0x0A0A are ordinary characters), an unterminated tail is a line, the empty document has
    none.  keep_ends=False: text is a NEW compacted buffer without any terminator unit and line_offsets index it; out / out_start: a
    caller-owned tensor of data's dtype, the result starting at its unit out_start (appending), units outside the result left as they are;
    text is then `out` itself, whole, as the gather entries return it (the result ends at line_offsets[-1]).
    keep_ends=True: a line includes its terminator, text is `data` itself and line_offsets are positions in it (out / out_start are not
    used).  line_offsets: int64[line_start + lines + 1], line j of the result at entries line_start + j and + 1, the entries in front equal
    to entry line_start; (text, line_offsets[line_start:]) goes into every *_packed method.  doc_line_offsets: int64[n + 1], document d
    gave the lines doc_line_offsets[d] .. doc_line_offsets[d + 1] (counted from line_start).
    needle_lines_count_packed_dev, torch cumsum, needle_lines_fill_packed_dev on one stream; the one host read is the two totals.  numpy
    inputs are uploaded and the results brought back (with out_start > 0 the out_start units in front of the result are not initialised, as
    in the gather entries' numpy form).  An empty input gives the empty batch without a call of the library."""
    import torch
    L = _lib.lib()
    if isinstance(data, np.ndarray):
        off = np.array([0, data.size], np.int64) if offsets is None else offsets
        d, (o,) = Pattern._gather_host_args(data, ((off, np.int64),))
        text, lo, dlo = lines_packed(d[:data.size], o, keep_ends, stream, None, out_start, line_start)
        host = np.ascontiguousarray(data)
        return host if keep_ends else Pattern._gather_host_text(text).view(host.dtype), lo.cpu().numpy(), dlo.cpu().numpy()
    Pattern._gather_check(data, ())
    dv, units = data.device, data.numel()
    if offsets is None:
        offsets = torch.tensor([0, units], dtype=torch.int64, device=dv)
    Pattern._gather_check(data, ((offsets, torch.int64, "offsets"),))
    n = offsets.numel() - 1
    assert n >= 0 and out_start >= 0 and line_start >= 0
    if out is not None:
        assert not keep_ends, "keep_ends: the text is data itself"
        assert out.device == dv and out.dtype == data.dtype and out.dim() == 1 and out.is_contiguous() and out.numel() >= out_start
    one = torch.cuda.current_stream(dv) if stream is None else torch.cuda.ExternalStream(stream, device=dv)
    with torch.cuda.device(dv), torch.cuda.stream(one):
        s = one.cuda_stream
        if n == 0 or units == 0:  # no line anywhere
            first = offsets[:1] if keep_ends else torch.full((1,), int(out_start), dtype=torch.int64, device=dv)
            text = data if keep_ends else (out if out is not None else torch.empty(out_start + 4, dtype=data.dtype, device=dv))[:out_start]
            return text, first.repeat(line_start + 1), torch.full((n + 1,), int(line_start), dtype=torch.int64, device=dv)
        v = _lib.PackedView()
        v.data, v.char_width, v.n_rows, v.offsets = data.data_ptr(), data.element_size(), n, offsets.data_ptr()
        flags = _lib.LINES_KEEP_ENDS if keep_ends else 0
        tiles = L.needle_lines_tiles(units, data.element_size())
        counts = torch.empty(2 * tiles, dtype=torch.int64, device=dv)
        bases = torch.empty(2 * (tiles + 1), dtype=torch.int64, device=dv)
        _check(L.needle_lines_count_packed_dev(ctypes.byref(v), units, flags, counts.data_ptr(), None if keep_ends else counts.data_ptr() + 8 * tiles, s))
        lb, ub = bases[:tiles + 1], bases[tiles + 1:]
        lb[0], ub[0] = int(line_start), int(out_start)
        torch.cumsum(counts[:tiles], 0, out=lb[1:])
        lb[1:] += int(line_start)
        if not keep_ends:
            torch.cumsum(counts[tiles:], 0, out=ub[1:])
            ub[1:] += int(out_start)
        line_end, unit_end = (int(x) for x in torch.stack([lb[-1], ub[-1]]).cpu())
        line_off = torch.empty(line_end + 1, dtype=torch.int64, device=dv)
        doc_off = torch.empty(n + 1, dtype=torch.int64, device=dv)
        if keep_ends:
            text, room = data, None
        elif out is None:
            room = torch.empty(unit_end + 4, dtype=data.dtype, device=dv)  # (never an empty allocation: its pointer would be NULL)
            text = room[:unit_end]
        else:
            assert out.numel() >= unit_end
            text = room = out
        _check(L.needle_lines_fill_packed_dev(ctypes.byref(v), units, flags, lb.data_ptr(), None if keep_ends else ub.data_ptr(), line_off.data_ptr(),
                                              None if keep_ends else room.data_ptr(), doc_off.data_ptr(), s))
        if line_start:
            line_off[:line_start] = line_off[line_start]
    return text, line_off, doc_off


def lines_of_bytes(buf, keep_ends=False):
    """bytes.splitlines(keep_ends) of `buf` on the device -> list[bytes]: upload, lines_packed, one download."""
    a = np.frombuffer(bytes(buf), dtype=np.uint8)
    text, off, _ = lines_packed(a, keep_ends=keep_ends)
    return [text[off[i]:off[i + 1]].tobytes() for i in range(off.size - 1)]


def unpack_bitmap(words, n_rows):
    """bitmap words -> bool array of n_rows (numpy)."""
    if not isinstance(words, np.ndarray):
        words = words.cpu().numpy()
    w = np.ascontiguousarray(words).view(np.uint64)
    bits = np.unpackbits(w.view(np.uint8), bitorder="little")
    return bits[:n_rows].astype(bool)


class DFACompiler:
    """DFACompiler.compile / compileToBytes entry point (DFACompiler.java:16-74): regex -> Pattern."""

    @staticmethod
    def compile(regex, class_name=None, flags=0):
        if regex is None:
            raise TypeError("regex string cannot be null")  # Objects.requireNonNull, RegexParser.java:87
        if flags & ~ALL_FLAGS:
            raise ValueError("Unknown flag bits")  # CompilerOptions.java:9-16
        u = _utf16(regex)
        h = ctypes.c_void_p()
        _check(_lib.lib().needle_compile(u.ctypes.data, u.size, int(flags), ctypes.byref(h)))
        return Pattern(h, regex, flags)
