"""CPU-side checks of the packed-row find() forms (needle_find_next_packed_dev, needle_find_packed{16,8}_packed_dev and _host):
exported, every argument check answers NEEDLE_ERR_INVALID before any device call, an empty batch returns NEEDLE_OK, a host batch
with a row beyond the form's limit is refused with NEEDLE_ERR_UNSUPPORTED before a device is touched, and the Python decoders
handle every escape -- none of this needs a GPU."""
import ctypes

import numpy as np
import pytest

DEV = ("needle_find_next_packed_dev", "needle_find_packed16_packed_dev", "needle_find_packed8_packed_dev")
HOST = ("needle_find_packed16_packed_host", "needle_find_packed8_packed_host")


@pytest.fixture(scope="module")
def lib():
    from needle_amd import build
    build.build()
    from needle_amd import _lib
    return _lib.lib()


@pytest.fixture(scope="module")
def pattern(lib):
    from needle_amd.pattern import DFACompiler
    return DFACompiler.compile("[0-9]+")


def test_symbols_exported(lib):
    from needle_amd import _lib
    for n in DEV + HOST:
        assert hasattr(lib, n), n
        assert n in _lib.EXPORTS, n


# host buffers stand in for device pointers: the calls must refuse before any of them is dereferenced or a device is used
_data = np.zeros(64, dtype=np.uint8)
_offsets = np.array([0, 3, 7], dtype=np.uint64)
_bm = np.zeros(1, dtype=np.uint64)
_a = np.zeros(2, dtype=np.int32)
_b = np.zeros(2, dtype=np.int32)
_cur = np.zeros(2, dtype=np.int32)
_ovf = np.zeros(1, dtype=np.int32)


def _view(data_ptr=None, cw=1, n=2, offsets_ptr=None, offsets=None):
    from needle_amd import _lib
    v = _lib.PackedView()
    v.data = _data.ctypes.data if data_ptr is None else data_ptr
    v.char_width, v.n_rows = cw, n
    v.offsets = (_offsets if offsets is None else offsets).ctypes.data if offsets_ptr is None else offsets_ptr
    return v


def _call(lib, name, h, v, bm=True, a=True, b=True, cur=True, ovf=True):
    bmp = _bm.ctypes.data if bm else None
    vp = ctypes.byref(v) if v is not None else None
    ap = _a.ctypes.data if a else None
    if name == "needle_find_next_packed_dev":
        return lib.needle_find_next_packed_dev(h, vp, _cur.ctypes.data if cur else None, bmp, ap, _b.ctypes.data if b else None, None)
    if name.endswith("_dev"):
        return getattr(lib, name)(h, vp, bmp, ap, _ovf.ctypes.data if ovf else None, None)
    return getattr(lib, name)(h, vp, bmp, ap)


@pytest.mark.parametrize("name", DEV + HOST)
def test_validation_without_device(lib, pattern, name):
    from needle_amd import _lib
    h = pattern._h
    bad = [
        (None, _view(), {}),                              # NULL pattern
        (h, None, {}),                                    # NULL view
        (h, _view(offsets_ptr=0), {}),                    # NULL offsets
        (h, _view(), {"bm": False}),                      # NULL bitmap
        (h, _view(), {"a": False}),                       # NULL results (start / the compact form)
        (h, _view(cw=0), {}),                             # char_width not 1 | 2
        (h, _view(cw=3), {}),
        (h, _view(cw=4), {}),
    ]
    if name.endswith("_dev"):
        bad += [(h, _view(data_ptr=_data.ctypes.data + 1), {}),   # data not 4-byte aligned
                (h, _view(data_ptr=_data.ctypes.data + 2, cw=2), {})]
    else:
        bad += [(h, _view(offsets=np.array([0, 7, 3], dtype=np.uint64)), {}),  # offsets decreasing
                (h, _view(data_ptr=0), {})]                                    # NULL data under a non-empty span
    if name == "needle_find_next_packed_dev":
        bad += [(h, _view(), {"cur": False}), (h, _view(), {"b": False})]
    for ph, v, kw in bad:
        assert _call(lib, name, ph, v, **kw) == _lib.ERR_INVALID, (name, kw)
        assert lib.needle_last_error()


@pytest.mark.parametrize("name", DEV + HOST)
def test_empty_batch_is_ok(lib, pattern, name):
    from needle_amd import _lib
    for cw in (1, 2):
        assert _call(lib, name, pattern._h, _view(cw=cw, n=0)) == _lib.NEEDLE_OK, (name, cw)


def test_overflow_flag_is_optional(lib, pattern):
    """The _dev compact forms take a NULL overflow pointer: only the outputs and the cursor are required (n_rows == 0: OK)."""
    from needle_amd import _lib
    for name in DEV[1:]:
        assert _call(lib, name, pattern._h, _view(n=0), ovf=False) == _lib.NEEDLE_OK, name


@pytest.mark.parametrize("name,limit", [("needle_find_packed16_packed_host", 65534), ("needle_find_packed8_packed_host", 256)])
def test_host_refuses_long_rows_before_the_device(lib, pattern, name, limit):
    """A row beyond the form's limit: NEEDLE_ERR_UNSUPPORTED (not NEEDLE_ERR_DEVICE on a machine without a GPU -- the check
    comes first), whatever its place in the batch and whatever offsets[0]; at the limit itself the offsets pass the check."""
    from needle_amd import _lib
    data = np.zeros(limit + 64, dtype=np.uint16)
    for offs, cw in (([0, 5, 5 + limit + 1], 1), ([3, 3 + limit + 1, 3 + limit + 2], 2), ([9, 9 + limit + 1], 1)):
        off = np.array(offs, dtype=np.uint64)
        v = _view(data_ptr=data.ctypes.data, cw=cw, n=off.size - 1, offsets=off)
        bm = np.zeros(1, np.uint64)
        out = np.zeros(off.size - 1, np.uint32)
        assert getattr(lib, name)(pattern._h, ctypes.byref(v), bm.ctypes.data, out.ctypes.data) == _lib.ERR_UNSUPPORTED, (name, offs)
        assert "rows of at most" in lib.needle_last_error().decode()
    # rows of exactly the limit pass the check: the call goes on to the device -- NEEDLE_OK where there is one (no match in these
    # zeros), NEEDLE_ERR_DEVICE where there is none -- and is neither refused nor rejected
    for offs, cw in (([0, limit], 1), ([3, 3 + limit], 2), ([0, 7, 7 + limit], 1)):
        off = np.array(offs, dtype=np.uint64)
        v = _view(data_ptr=data.ctypes.data, cw=cw, n=off.size - 1, offsets=off)
        bm = np.full(1, 7, np.uint64)
        out = np.zeros(off.size - 1, np.uint32)
        rc = getattr(lib, name)(pattern._h, ctypes.byref(v), bm.ctypes.data, out.ctypes.data)
        assert rc in (_lib.NEEDLE_OK, _lib.ERR_DEVICE), (name, offs, rc, lib.needle_last_error())
        if rc == _lib.NEEDLE_OK:
            assert int(bm[0]) == 0, (name, offs)


def test_python_entries_exist():
    import inspect
    from needle_amd.pattern import Pattern
    assert list(inspect.signature(Pattern.find_next_packed).parameters) == ["self", "data", "offsets", "cursor", "stream"]
    for m in ("find_packed16_packed", "find_packed8_packed"):
        assert list(inspect.signature(getattr(Pattern, m)).parameters) == ["self", "data", "offsets", "stream", "out"], m


def test_python_numpy_host_path_refuses_long_rows(pattern):
    """numpy inputs take the _host entries: the limit check answers (PatternException-like error) without a device."""
    from needle_amd import _lib
    data = np.zeros(300, np.uint8)
    with pytest.raises(Exception) as ei:
        pattern.find_packed8_packed(data, np.array([0, 1, 300], np.int64))
    assert "256" in str(ei.value)


def test_escape_constants_match_the_header():
    import os
    import re
    from needle_amd.pattern import PACK16_OVER, PACK8_OVER
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "needle_hip.h")).read()
    assert int(re.search(r"#define NEEDLE_PACK16_OVER (0x[0-9A-Fa-f]+)u", hdr).group(1), 16) == PACK16_OVER
    assert int(re.search(r"#define NEEDLE_PACK8_OVER (0x[0-9A-Fa-f]+)u", hdr).group(1), 16) == PACK8_OVER


def test_unpack16_packed_every_escape():
    from needle_amd.pattern import Pattern, PACK16_OVER
    x = np.array([0xFFFFFFFF, PACK16_OVER, 0 | 0 << 16, 3 | 9 << 16, 0 | 65534 << 16, 65533 | 65534 << 16, 7 | 7 << 16], np.uint32)
    for arr in (x, x.view(np.int32), x.astype(np.int64)):
        s, e, over = Pattern.unpack16_packed(arr)
        assert s.tolist() == [-1, -1, 0, 3, 0, 65533, 7]
        assert e.tolist() == [-1, -1, 0, 9, 65534, 65534, 7]
        assert over.tolist() == [False, True, False, False, False, False, False]
    # the escape cannot collide with a held match: start 0xFFFF > end 0xFFFE
    assert (PACK16_OVER & 0xFFFF) > (PACK16_OVER >> 16)


def test_unpack8_packed_every_escape():
    from needle_amd.pattern import Pattern, PACK8_OVER
    x = np.array([0xFFFF, 0xFFFE, PACK8_OVER, 0, 5 | 3 << 8, 255 | 1 << 8, 0 | 255 << 8, 1 | 255 << 8], np.uint16)
    for arr in (x, x.view(np.int16), x.astype(np.int32)):
        s, e, over = Pattern.unpack8_packed(arr)
        assert s.tolist() == [-1, 0, -1, 0, 5, 255, 0, 1]
        assert e.tolist() == [-1, 256, -1, 0, 8, 256, 255, 256]
        assert over.tolist() == [False, False, True, False, False, False, False, False]
    # no held match (start + length <= 256) encodes 0xFFFD, 0xFFFE or 0xFFFF
    held = {(s | (l << 8)) for s in range(257) for l in range(256) if s + l <= 256 and s < 256}
    assert not held & {PACK8_OVER, 0xFFFE, 0xFFFF}
    # the existing decoder is unchanged
    s8, e8 = Pattern.unpack8(np.array([0xFFFF, 0xFFFE, 5 | 3 << 8], np.uint16))
    assert s8.tolist() == [-1, 0, 5] and e8.tolist() == [-1, 256, 8]
